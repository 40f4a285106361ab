"""The reference of the SSIM / MS-SSIM pair kernel in plain fp64 numpy, one pair at a time, and seeded inputs.

Per channel c and level l on planes x, y (level 0: the bytes as numbers): g_j = exp(-(j - 5)^2 / 4.5) / sum, j = 0..10, separable, over
the valid region; mx, my, exx, eyy, exy the windowed means of x, y, x x, y y, x y; vx = exx - mx mx, vy = eyy - my my, vxy = exy - mx my;
cs_map = (2 vxy + C2) / (vx + vy + C2); ss_map = (2 mx my + C1) / (mx mx + my my + C1) * cs_map; cs[c][l], ss[c][l] their means; the
next level is the 2 x 2 mean.  ssim = mean_c ss[c][0]; ms[c] = prod_{l<L-1} max(cs[c][l], 0)^w_l * max(ss[c][L-1], 0)^w_(L-1) with w the
first L of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) over their sum; ms_ssim = mean_c ms[c]; sq_err = sum (a - b)^2."""
import functools

import numpy as np

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TOL = 5e-5                     # fp32 emulation of the definition against fp64: at most 9.0e-6 on these inputs; 5x for the order of addition


def window():
    g = np.array([np.exp(-((j - 5) ** 2) / 4.5) for j in range(11)], dtype=np.float64)
    return g / g.sum()


@functools.lru_cache(maxsize=None)
def band(s):
    """[s-10, s]: G[o][o + j] = g_j, the window over the valid region as a matrix"""
    G = np.zeros((s - 10, s))
    for o in range(s - 10):
        G[o, o:o + 11] = window()
    return G


def blur(p):
    """[s,s] -> [s-10,s-10]: the window along both axes over the valid region"""
    G = band(p.shape[0])
    return G @ p @ G.T


def level_terms(x, y):
    mx, my = blur(x), blur(y)
    vx, vy, vxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    cs = (2 * vxy + C2) / (vx + vy + C2)
    ss = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
    return cs.mean(), ss.mean()


def halve(p):
    s = p.shape[0] // 2
    return p.reshape(s, 2, s, 2).mean(axis=(1, 3))


def weights(L):
    w = np.array(WEIGHTS[:L], dtype=np.float64)
    return w / w.sum()


def combine(terms):
    """(ssim, ms_ssim) of one pair from terms [3][L][2]"""
    t = np.asarray(terms, dtype=np.float64)
    L = t.shape[1]
    w = weights(L)
    ms = []
    for c in range(3):
        v = 1.0
        for l in range(L):
            v *= max(t[c, l, 1 if l == L - 1 else 0], 0.0) ** w[l]
        ms.append(v)
    return float(t[:, 0, 1].mean()), float(np.mean(ms))


def pair_ref(a, b, L):
    """one pair of uint8 [S,S,3] -> (terms fp64 [3,L,2], ssim, ms_ssim, sq_err int)"""
    t = np.empty((3, L, 2))
    for c in range(3):
        x, y = a[:, :, c].astype(np.float64), b[:, :, c].astype(np.float64)
        for l in range(L):
            t[c, l] = level_terms(x, y)
            if l + 1 < L:
                x, y = halve(x), halve(y)
    ssim, ms = combine(t)
    d = a.astype(np.int64) - b.astype(np.int64)
    return t, ssim, ms, int((d * d).sum())


def pairs_ref(a, b, ia, ib, L):
    """{"terms" [P,3,L,2], "ssim", "ms_ssim" fp64 [P], "sq_err" int64 [P]} of index lists inside their arrays"""
    res = [pair_ref(a[i], b[j], L) for i, j in zip(ia, ib)]
    return {"terms": np.stack([r[0] for r in res]), "ssim": np.array([r[1] for r in res]), "ms_ssim": np.array([r[2] for r in res]),
            "sq_err": np.array([r[3] for r in res], dtype=np.int64)}


# ---- seeded inputs: uint8 [n,S,S,3]
def smooth(n, S, seed):
    """block noise x 8 plus pixel noise.  Half of every block's level is common to the n pictures, as the samples of one class share
    their layout: the structure terms of two of them then lie well away from zero at every level"""
    g = np.random.default_rng(seed)
    cells = (S + 7) // 8
    blocks = (g.integers(30, 226, size=(1, cells, cells, 3)) + g.integers(30, 226, size=(n, cells, cells, 3))) // 2
    base = np.repeat(np.repeat(blocks, 8, axis=1), 8, axis=2)[:, :S, :S]
    return np.clip(base + g.integers(-12, 13, size=(n, S, S, 3)), 0, 255).astype(np.uint8)


def noise(n, S, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, S, S, 3), dtype=np.uint8)


def flat_pair(S):
    """[2]: all 250, and the same with one pixel 251"""
    x = np.full((2, S, S, 3), 250, np.uint8)
    x[1, S // 2, S // 3, :] = 251
    return x


def extremes(S):
    """[2]: all 255, all 0"""
    x = np.zeros((2, S, S, 3), np.uint8)
    x[0] = 255
    return x


def jitter(img, seed):
    """the picture with +-2 added to every byte (clipped)"""
    g = np.random.default_rng(seed)
    return np.clip(img.astype(np.int64) + g.choice([-2, 2], size=img.shape), 0, 255).astype(np.uint8)


def blend(a, b):
    """the 50 % blend of two pictures (rounded half up)"""
    return ((a.astype(np.int64) + b.astype(np.int64) + 1) // 2).astype(np.uint8)


def case_set(S, seed):
    """the input kinds in one array and the pairs worth comparing: (uint8 [15,S,S,3], ia, ib, smooth_like bool [46])
    0-6 smooth, 7 noise, 8 / 9 flat 250 and one pixel 251, 10 / 11 all 255 and all 0, 12 jitter of 0, 13 / 14 blends of 1, 2 and of 3, 4.
    The first 40 pairs are among the smooth pictures, their jitter and their blends; then picture against noise, noise against jitter,
    the flat pair, the extremes and two pictures against themselves."""
    sm = smooth(7, S, seed)
    x = np.concatenate([sm, noise(1, S, seed + 1), flat_pair(S), extremes(S), jitter(sm[0], seed + 2)[None], blend(sm[1], sm[2])[None],
                        blend(sm[3], sm[4])[None]])
    like = (0, 1, 2, 3, 4, 5, 6, 12, 13, 14)
    pairs = [(i, j) for n, i in enumerate(like) for j in like[n + 1:]][:40] + [(0, 7), (7, 12), (8, 9), (10, 11), (3, 3), (7, 7)]
    ia, ib = (np.array(v, dtype=np.int64) for v in zip(*pairs))
    return x, ia, ib, np.arange(len(pairs)) < 40
