"""Host side of the power spectra of pictures (Durall et al. 2020, Dzanic et al. 2020, Odena et al. 2016):

    a = metrics.spectrum(samples_u8, mean2d=True)      # {"profile" [n][R], "mean" [n], "radius", "count", "mean2d" [S][S], ...}
    b = metrics.spectrum(train_u8, mean2d=True)        # csrc/spectrum.hip on CUDA tensors, numpy fp64 (here) otherwise
    r = metrics.spectrum_report(a, b)                  # gaps in dB per radial bin, lattice peaks, checkerboard_db, separability
    print(format_report(r))

Here: the plane names, the periodic Hann window table, the integer radial bin map and its counts, the fp64 numpy path that
metrics.spectrum's host path is made of, the report, the lattice points and the rendering of a mean plane for the sheet.  How the numbers
read: `gap_db[r]` is the samples' mean log power minus the training set's at radius r (0 = the mean level, S / 2 = the axis Nyquist, the
last bin the corner (S/2, S/2)); a generator of stride-2 transposed convolutions typically bends away at high radius (`high_gap_db`) and
leaves peaks on the lattice (a S/4, b S/4), the corner one being the checkerboard (`checkerboard_db`)."""
import numpy as np

from ._lib import JckError

SIZES = (32, 64, 128)
PLANES = ("r", "g", "b", "luma")
WINDOWS = (None, "hann")
LUMA = (77, 150, 29)                       # / 256
DB_FLOOR = 1e-6                            # profiles are clamped here before the logarithm (the 8-bit quantisation floor is near 1/12)
RENDER_DB = (-20.0, 50.0)                  # render(): 10 log10 P over this range -> 0..255
RENDER_DIFF_DB = (-10.0, 10.0)             # render_diff(): the difference of two planes in dB over this range -> 0..255


def plane_index(plane):
    """"r" / "g" / "b" / "luma" or 0..3 -> 0..3"""
    if isinstance(plane, str):
        if plane not in PLANES:
            raise ValueError(f"spectrum: plane = {plane!r} must be one of {PLANES} (or 0..3)")
        return PLANES.index(plane)
    if isinstance(plane, (bool, np.bool_)) or not isinstance(plane, (int, np.integer)) or not 0 <= int(plane) <= 3:
        raise ValueError(f"spectrum: plane = {plane!r} must be one of {PLANES} (or 0..3)")
    return int(plane)


def check_window(window):
    if window not in WINDOWS:
        raise ValueError(f"spectrum: window = {window!r} must be None or 'hann'")
    return window


def hann(S):
    """the periodic Hann window 0.5 - 0.5 cos(2 pi j / S), computed in fp64 and rounded to fp32 [S]"""
    j = np.arange(int(S), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * j / int(S))).astype(np.float32)


def window_table(S, window):
    """(fp32 [S] or None, the window power W = (sum_j w[j]^2 / S)^2 in fp64 from the rounded table; 1 without a window)"""
    if check_window(window) is None:
        return None, 1.0
    w = hann(S)
    return w, float((w.astype(np.float64) ** 2).sum() / int(S)) ** 2


def bin_map(S):
    """int [S][S]: the bin r of (u, v), the unique integer with r^2 - r < d2 <= r^2 + r for d2 = min(u, S-u)^2 + min(v, S-v)^2 (r = 0
    at d2 = 0): floor(sqrt(d2) + 0.5) in integers only"""
    S = int(S)
    f = np.minimum(np.arange(S), S - np.arange(S)).astype(np.int64)
    d2 = f[:, None] ** 2 + f[None, :] ** 2
    r = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)           # a start; the integer rule decides
    r = np.where(r * r + r < d2, r + 1, r)
    r = np.where(r * r - r >= d2, r - 1, r)
    r = np.where(d2 == 0, 0, r)
    assert ((r * r - r < d2) & (d2 <= r * r + r) | (d2 == 0)).all()
    return r


def bins(S):
    """R = 24 / 46 / 92 for S = 32 / 64 / 128 (the corners count)"""
    if int(S) not in SIZES:
        raise JckError(f"spectrum: S = {S} must be one of {SIZES}")
    return int(bin_map(S).max()) + 1


def counts(S):
    """int64 [R]: the number of (u, v) in each bin"""
    return np.bincount(bin_map(S).reshape(-1), minlength=bins(S)).astype(np.int64)


def plane_values(u8, plane):
    """uint8 [n,S,S,3] -> the integer Y [n,S,S] (int64): 77 R + 150 G + 29 B for luma, 256 * byte for a channel"""
    x = np.asarray(u8)
    p = plane_index(plane)
    if p == 3:
        return LUMA[0] * x[..., 0].astype(np.int64) + LUMA[1] * x[..., 1].astype(np.int64) + LUMA[2] * x[..., 2].astype(np.int64)
    return 256 * x[..., p].astype(np.int64)


def power_planes(u8, plane="luma", window=None):
    """fp64 numpy of the definition: (P [n][S][S], mean [n]) - the centred plane (S^2 Y - T) / (256 S^2), the fp32 window table applied
    in fp64, np.fft.fft2, |F|^2 / (S^2 W)"""
    Y = plane_values(u8, plane)
    n, S = Y.shape[0], Y.shape[1]
    T = Y.reshape(n, -1).sum(axis=1)
    val = (S * S * Y - T[:, None, None]).astype(np.float64) / (256.0 * S * S)
    w, W = window_table(S, window)
    if w is not None:
        w = w.astype(np.float64)
        val = val * w[None, :, None] * w[None, None, :]
    F = np.fft.fft2(val, axes=(1, 2))
    return (F.real ** 2 + F.imag ** 2) / (S * S * W), T.astype(np.float64) / (256.0 * S * S)


def profile_of(P):
    """fp64 [n][S][S] -> [n][R]: the mean of P over each bin"""
    n, S = P.shape[0], P.shape[1]
    b, c = bin_map(S).reshape(-1), counts(S)
    out = np.zeros((n, c.shape[0]))
    flat = P.reshape(n, -1)
    for i in range(n):
        out[i] = np.bincount(b, weights=flat[i], minlength=c.shape[0]) / c
    return out


def result(profile, mean, S, plane, window, mean2d=None):
    """the dict metrics.spectrum returns"""
    return {"profile": np.asarray(profile, np.float64), "mean": np.asarray(mean, np.float64), "radius": np.arange(bins(S), dtype=np.int64),
            "count": counts(S), "mean2d": mean2d, "S": int(S), "plane": PLANES[plane_index(plane)], "window": check_window(window)}


def host_spectrum(u8, plane, window, mean2d, chunk):
    """the numpy path, `chunk` pictures at a time (the [n][S][S] fp64 planes of a large set need not exist at once)"""
    x = np.asarray(u8)
    n, S = int(x.shape[0]), int(x.shape[1])
    prof, mean, total = np.zeros((n, bins(S))), np.zeros(n), np.zeros((S, S))
    for lo in range(0, n, chunk):
        P, m = power_planes(x[lo:lo + chunk], plane, window)
        prof[lo:lo + chunk], mean[lo:lo + chunk] = profile_of(P), m
        if mean2d:
            total += P.sum(axis=0)
    return result(prof, mean, S, plane, window, (total / max(n, 1)) if mean2d else None)


# ---- the report ----------------------------------------------------------------------------------------------------------------------
def to_db(profile):
    return 10.0 * np.log10(np.maximum(np.asarray(profile, np.float64), DB_FLOOR))


def lattice_points(S):
    """the 15 (a S/4, b S/4), a, b in 0..3, without (0, 0)"""
    q = int(S) // 4
    return [(a * q, b * q) for a in range(4) for b in range(4) if (a, b) != (0, 0)]


def peak_db(mean2d, u, v):
    """10 log10(mean2d[u][v] / the median of the 24 other points of its wrapped 5 x 5 neighbourhood)"""
    m = np.asarray(mean2d, np.float64)
    S = m.shape[0]
    around = [m[(u + du) % S, (v + dv) % S] for du in range(-2, 3) for dv in range(-2, 3) if (du, dv) != (0, 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(m[u, v] / np.median(around)))


def _set_stats(s):
    db = to_db(s["profile"])
    n = db.shape[0]
    return db, db.mean(axis=0), (db.std(axis=0, ddof=1) if n > 1 else np.zeros(db.shape[1])), n


def separability(db_a, db_b):
    """AUROC (hipgan.anomaly.auroc) on the odd-indexed rows of a diagonal-covariance linear discriminant fitted on the even-indexed rows
    of both sets; None below 4 pictures a set.  0.5: a linear rule on the R numbers cannot tell the sets apart."""
    from .anomaly import auroc
    if db_a.shape[0] < 4 or db_b.shape[0] < 4:
        return None
    fa, fb, ta, tb = db_a[0::2], db_b[0::2], db_a[1::2], db_b[1::2]
    ma, mb = fa.mean(axis=0), fb.mean(axis=0)
    var = (((fa - ma) ** 2).sum(axis=0) + ((fb - mb) ** 2).sum(axis=0)) / max(fa.shape[0] + fb.shape[0] - 2, 1)
    w = np.where(var > 0, (ma - mb) / np.where(var > 0, var, 1.0), 0.0)
    if not np.any(w):
        return 0.5
    mid = 0.5 * (ma + mb)
    scores = np.concatenate([(ta - mid) @ w, (tb - mid) @ w])
    return float(auroc(scores, np.arange(scores.shape[0]) < ta.shape[0]))


def report(a, b):
    """two metrics.spectrum dicts (A: samples, B: training pictures; one S, plane and window) -> the report dict of DESIGN 5.18"""
    for k in ("S", "plane", "window"):
        if a[k] != b[k]:
            raise ValueError(f"spectrum_report: the two sets differ in {k}: {a[k]!r} and {b[k]!r}")
    S = int(a["S"])
    if a["profile"].shape[0] < 1 or b["profile"].shape[0] < 1:
        raise ValueError(f"spectrum_report: a set is empty ({a['profile'].shape[0]} and {b['profile'].shape[0]} pictures)")
    db_a, mean_a, std_a, na = _set_stats(a)
    db_b, mean_b, std_b, nb = _set_stats(b)
    gap = mean_a - mean_b
    root = np.sqrt(std_a ** 2 / na + std_b ** 2 / nb)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(root > 0, gap / np.where(root > 0, root, 1.0), np.where(gap == 0, 0.0, np.sign(gap) * np.inf))
    R = gap.shape[0]
    worst = int(np.argmax(np.abs(gap)))
    out = {"S": S, "plane": a["plane"], "window": a["window"], "n_a": na, "n_b": nb, "radius": np.arange(R, dtype=np.int64), "count": counts(S),
           "mean_db_a": mean_a, "std_db_a": std_a, "mean_db_b": mean_b, "std_db_b": std_b, "gap_db": gap, "z": z,
           "rms_gap_db": float(np.sqrt((gap[1:] ** 2).mean())), "high_gap_db": float(gap[np.arange(R) > S // 4].mean()),
           "worst": {"bin": worst, "gap_db": float(gap[worst]), "z": float(z[worst])},
           "separability": separability(db_a, db_b), "peaks": None, "checkerboard_db": None,
           "mean2d_a": a.get("mean2d"), "mean2d_b": b.get("mean2d")}
    if a.get("mean2d") is not None and b.get("mean2d") is not None:
        peaks = []
        for u, v in lattice_points(S):
            pa, pb = peak_db(a["mean2d"], u, v), peak_db(b["mean2d"], u, v)
            peaks.append({"u": u, "v": v, "a_db": pa, "b_db": pb, "diff_db": pa - pb})
        out["peaks"] = peaks
        out["checkerboard_db"] = next(p["diff_db"] for p in peaks if (p["u"], p["v"]) == (S // 2, S // 2))
    return out


def format_report(r):
    sep = "n/a" if r["separability"] is None else f"{r['separability']:.3f}"
    cb = "n/a" if r["checkerboard_db"] is None else f"{r['checkerboard_db']:+.2f} dB"
    w = r["worst"]
    return (f"rms gap {r['rms_gap_db']:.2f} dB | high-frequency gap {r['high_gap_db']:+.2f} dB | worst bin {w['bin']} {w['gap_db']:+.2f} dB (z {w['z']:+.1f}) | "
            f"checkerboard {cb} | separability {sep}")


def _num(v):
    v = float(v)
    return v if np.isfinite(v) else (None if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def to_json(r):
    """the JSON form of a report: the summary, the peaks and the settings (the per-bin arrays and the planes go to the .npz)"""
    out = {"S": r["S"], "plane": r["plane"], "window": r["window"], "n_a": r["n_a"], "n_b": r["n_b"], "bins": int(r["gap_db"].shape[0]),
           "rms_gap_db": _num(r["rms_gap_db"]), "high_gap_db": _num(r["high_gap_db"]),
           "worst": {"bin": r["worst"]["bin"], "gap_db": _num(r["worst"]["gap_db"]), "z": _num(r["worst"]["z"])},
           "separability": r["separability"], "checkerboard_db": None if r["checkerboard_db"] is None else _num(r["checkerboard_db"]), "peaks": None}
    if r["peaks"] is not None:
        out["peaks"] = [{"u": p["u"], "v": p["v"], "a_db": _num(p["a_db"]), "b_db": _num(p["b_db"]), "diff_db": _num(p["diff_db"])} for p in r["peaks"]]
    for k in ("n", "n_train", "seed"):
        if k in r:
            out[k] = r[k]
    return out


def arrays_of(r, suffix=""):
    """the .npz arrays of a report"""
    out = {k + suffix: np.asarray(r[k]) for k in ("radius", "count", "mean_db_a", "std_db_a", "mean_db_b", "std_db_b", "gap_db", "z")}
    for k in ("mean2d_a", "mean2d_b"):
        if r.get(k) is not None:
            out[k + suffix] = np.asarray(r[k])
    return out


def _to_u8(x, lo, hi):
    return np.clip(np.rint((np.asarray(x, np.float64) - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)


def render(mean2d, db_range=RENDER_DB):
    """uint8 [S][S][3] (grey): 10 log10 of the fft-shifted plane (zero frequency at the centre; floored at DB_FLOOR) mapped linearly from
    db_range = (-20, 50) dB to 0..255"""
    g = _to_u8(to_db(np.fft.fftshift(np.asarray(mean2d, np.float64))), *db_range)
    return np.repeat(g[:, :, None], 3, axis=2)


def render_diff(mean2d_a, mean2d_b, db_range=RENDER_DIFF_DB):
    """uint8 [S][S][3]: the dB difference A - B of two fft-shifted planes over db_range = (-10, 10) dB; mid grey = equal, the samples'
    excess towards red, their deficit towards blue"""
    d = np.fft.fftshift(to_db(mean2d_a) - to_db(mean2d_b))
    lo, hi = db_range
    t = np.clip((d - lo) / (hi - lo), 0.0, 1.0)                                  # 0.5 = equal
    up, dn = np.clip(2 * t - 1, 0, 1), np.clip(1 - 2 * t, 0, 1)
    rgb = np.stack([128 + 127 * up - 128 * dn, 128 - 128 * up - 128 * dn, 128 - 128 * up + 127 * dn], axis=2)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
