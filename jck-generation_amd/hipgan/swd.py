"""Host helpers of the sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, section 5):

    r = metrics.swd(a_u8, b_u8)                 # {"swd" [L] (x 1e3), "mean", "sides", "per_repeat" [R][L]}; csrc/swd.hip on CUDA tensors
    print(format_report(r))                     # 64x64 12.31 | 32x32 9.87 | 16x16 30.02 | mean 17.40

Here: the level geometry, the seeded draw of the patch corners and the directions, the fp64 numpy pyramid and descriptors that
metrics.swd's host path is made of, and the report dict.  A level's number says how far the statistics of 7 x 7 neighbourhoods of the
two sets are apart at that scale: the finest level reads as texture and noise, the middle ones as shapes, the coarsest (the low-pass
picture itself, not a band) as layout and colour."""
import numpy as np

from ._lib import JckError

SIZES = (32, 64, 128)
PATCH, DESC = 7, 147
MIN_SIDE = 16
READS_AS = {128: "fine texture, noise", 64: "texture", 32: "shapes", 16: "layout, colour"}
_W = np.array([1.0, 4.0, 6.0, 4.0, 1.0])


def max_levels(S):
    """the number of levels S >> l with side >= 16 for S in SIZES, 0 for another S (jck_swd_max_levels gives the same)"""
    S = int(S)
    return 0 if S not in SIZES else S.bit_length() - 4


def sides(S, L):
    return [int(S) >> l for l in range(int(L))]


def level_names(S, L):
    return [f"{s}x{s}" for s in sides(S, L)]


def draw(n, S, L, patches=128, dirs=128, repeats=4, seed=0):
    """(pos int32 [n][L][P][2] = (y, x) in [0, s_l - 7], dirs fp32 [R][D][147] of unit length) from numpy.random.default_rng(seed):
    the corners level by level, then the directions (standard normal, scaled to unit length in fp64, rounded to fp32)"""
    n, L, P, D, R = int(n), int(L), int(patches), int(dirs), int(repeats)
    if n < 1 or P < 1 or D < 1 or R < 1 or not 1 <= L <= max_levels(S):
        raise JckError(f"swd.draw: n = {n}, patches = {P}, dirs = {D}, repeats = {R} must be >= 1 and levels = {L} in 1..{max_levels(S)} at S = {S}")
    g = np.random.default_rng(int(seed))
    pos = np.stack([g.integers(0, (int(S) >> l) - PATCH + 1, size=(n, P, 2)) for l in range(L)], axis=1).astype(np.int32)
    d = g.standard_normal((R, D, DESC))
    d /= np.sqrt((d * d).sum(axis=2, keepdims=True))
    return pos, d.astype(np.float32)


def _filter(x, w, axis):
    """the 5-tap filter w along `axis` with mirror borders (numpy reflect: the edge sample is not repeated)"""
    pad = [(0, 0)] * x.ndim
    pad[axis] = (2, 2)
    xp = np.pad(x, pad, mode="reflect")
    n = x.shape[axis]
    return sum(w[k] * np.take(xp, np.arange(k, k + n), axis=axis) for k in range(5))


def down(g):
    """[..., s, s] -> [..., s/2, s/2]: binomial [1,4,6,4,1] / 16 in both axes, then the even samples"""
    return _filter(_filter(g, _W / 16.0, -1), _W / 16.0, -2)[..., ::2, ::2]


def up(x):
    """[..., m, m] -> [..., 2m, 2m]: the samples at the even positions, zeros elsewhere, then [1,4,6,4,1] / 8 in both axes"""
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]), dtype=x.dtype)
    z[..., ::2, ::2] = x
    return _filter(_filter(z, _W / 8.0, -1), _W / 8.0, -2)


def pyramid(u8, L):
    """uint8 [n,S,S,3] -> (G, Lap): lists of fp64 [n,3,s_l,s_l]; Lap_l = G_l - up(G_(l+1)), Lap_(L-1) = G_(L-1)"""
    g = [np.moveaxis(np.asarray(u8), 3, 1).astype(np.float64)]
    for _ in range(1, L):
        g.append(down(g[-1]))
    return g, [g[l] - up(g[l + 1]) for l in range(L - 1)] + [g[L - 1]]


def descriptors(plane, pos_l):
    """[n,3,s,s], corners [n,P,2] -> [n*P, 3, 49]: the 7 x 7 x 3 patches in the order [c][dy][dx]"""
    n, P = pos_l.shape[:2]
    k = np.arange(PATCH)
    yy = pos_l[:, :, 0, None, None] + k[None, None, :, None]
    xx = pos_l[:, :, 1, None, None] + k[None, None, None, :]
    d = plane[np.arange(n)[:, None, None, None], :, yy, xx]                         # [n,P,7,7,3]
    return np.ascontiguousarray(np.moveaxis(d, 4, 2)).reshape(n * P, 3, PATCH * PATCH)


def moments(d):
    """(mean [3], rstd [3]) over every component of a channel (population); rstd = 0 where the deviation is 0"""
    mean, std = d.mean(axis=(0, 2)), d.std(axis=(0, 2))
    return mean, np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)


def moments_from_sums(total, total_sq, count):
    """the same from sum and sum of squares [..]: var = sumsq / N - mean^2, rstd = 0 where var <= 0"""
    mean = np.asarray(total, np.float64) / count
    var = np.asarray(total_sq, np.float64) / count - mean * mean
    return mean, np.where(var > 0, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 0.0)


def report(per_repeat, S, settings=None):
    """per_repeat fp64 [R][L] (already x 1e3) -> {"swd" [L], "mean", "sides", "per_repeat"} (+ settings)"""
    pr = np.asarray(per_repeat, dtype=np.float64)
    out = {"swd": pr.mean(axis=0), "sides": sides(S, pr.shape[1]), "per_repeat": pr}
    out["mean"] = float(out["swd"].mean())
    if settings:
        out.update(settings)
    return out


def format_report(r):
    return " | ".join(f"{s}x{s} {v:.2f}" for s, v in zip(r["sides"], r["swd"])) + f" | mean {r['mean']:.2f}"


def to_json(r):
    """the JSON form of a report: lists and floats (per_repeat goes to the .npz)"""
    out = {k: v for k, v in r.items() if k not in ("per_repeat", "per_class")}
    out["swd"] = [float(v) for v in r["swd"]]
    out["levels"] = level_names(r["sides"][0], len(r["sides"]))
    out["reads_as"] = [READS_AS.get(s, "") for s in r["sides"]]
    return out
