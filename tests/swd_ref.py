"""fp64 numpy restatement of the sliced Wasserstein distance on Laplacian-pyramid patches, written from the definition
and sharing no code with metrics.swd or hipgan.swd: the filters are whole-plane np.pad(mode="reflect") and shifted slices, the
descriptors are cut patch by patch, the directions are applied one dot product layout at a time."""
import numpy as np

W5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])


def blur(x, w):
    """[.., h, w] filtered with the 5 taps w in both axes, mirror borders"""
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)], mode="reflect")
    h, wd = x.shape[-2:]
    rows = sum(w[k] * p[..., k:k + h, :] for k in range(5))
    return sum(w[k] * rows[..., :, k:k + wd] for k in range(5))


def down(g):
    return blur(g, W5 / 16.0)[..., 0::2, 0::2]


def up(x):
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]))
    z[..., 0::2, 0::2] = x
    return blur(z, W5 / 8.0)


def levels_of(S):
    L = 1
    while (S >> L) >= 16:
        L += 1
    return L


def pyramid(u8, L):
    """uint8 [n,S,S,3] -> (G, Lap), lists of fp64 [n,3,s,s]"""
    g = [np.transpose(u8.astype(np.float64), (0, 3, 1, 2))]
    for _ in range(L - 1):
        g.append(down(g[-1]))
    lap = [g[l] - up(g[l + 1]) for l in range(L - 1)] + [g[L - 1]]
    return g, lap


def descriptors(plane, pos_l):
    """[n,3,s,s], corners [n,P,2] (y, x) -> fp64 [n,P,147] in the order [c][dy][dx]"""
    n, P = pos_l.shape[:2]
    out = np.empty((n, P, 147))
    for i in range(n):
        for p in range(P):
            y, x = int(pos_l[i, p, 0]), int(pos_l[i, p, 1])
            out[i, p] = plane[i, :, y:y + 7, x:x + 7].reshape(147)
    return out


def stats(desc):
    """fp64 [n,P,147] -> (sum [3], sumsq [3], mean [3], rstd [3]) per channel, population deviation, rstd 0 at zero deviation"""
    d = desc.reshape(-1, 3, 49)
    mean = d.mean(axis=(0, 2))
    dev = np.sqrt(((d - mean[None, :, None]) ** 2).mean(axis=(0, 2)))
    rstd = np.array([1.0 / v if v > 0 else 0.0 for v in dev])
    return d.sum(axis=(0, 2)), (d * d).sum(axis=(0, 2)), mean, rstd


def normalise(desc, mean, rstd):
    d = desc.reshape(desc.shape[0], desc.shape[1], 3, 49)
    return ((d - mean[None, None, :, None]) * rstd[None, None, :, None]).reshape(desc.shape)


def project(xn, dirs):
    """normalised fp64 [n,P,147], dirs [D,147] -> [D][n*P]"""
    return np.einsum("ipk,dk->dip", xn, dirs.astype(np.float64)).reshape(dirs.shape[0], -1)


def swd(a, b, pos, dirs, L):
    """a, b uint8 [n,S,S,3]; pos [n,L,P,2]; dirs fp32 [R,D,147] -> per_repeat [R][L] (x 1e3)"""
    la, lb = pyramid(a, L)[1], pyramid(b, L)[1]
    out = np.zeros((dirs.shape[0], L))
    for l in range(L):
        xs = []
        for lap in (la, lb):
            d = descriptors(lap[l], pos[:, l])
            _, _, mean, rstd = stats(d)
            xs.append(normalise(d, mean, rstd))
        for r in range(dirs.shape[0]):
            pa, pb = np.sort(project(xs[0], dirs[r]), axis=1), np.sort(project(xs[1], dirs[r]), axis=1)
            out[r, l] = 1e3 * np.mean(np.mean(np.abs(pa - pb), axis=1))
    return out


def device_error_bound(a, b, pos, dirs, L):
    """[L]: how far an element of the device path's projections may lie from the fp64 ones of the same pictures, corners and directions,
    the larger of the two sets.  With m, r the channel's mean and 1 / deviation, u = 2^-24, per element sum over the 147 components of
        (60 + |m r| + 3 (m r)^2) u (|x_i| + |m|) r |d_i|  +  2 u (1 + |m| r) |d_i|
    - 53 u sum |(x_i - m) r d_i| is the kernel's own chain (49 + 2 additions, two roundings of the normalisation: csrc/swd.hip), and
      |(x_i - m) r d_i| <= (|x_i| + |m|) r |d_i|;
    - one u on |x_i| r |d_i| for the descriptor's single rounding to fp32;
    - the device takes m and r from the ROUNDED descriptors and hands them over in fp32: |dm| <= u (mean |x| + |m|) <= u (1 / r + 2 |m|)
      (mean |x| <= sqrt(mean x^2) <= 1 / r + |m|), which moves an element by at most 2 u (1 + |m| r) |d_i| per component;
    - the variance mean(x^2) - m^2 moves by at most 2 u mean(x^2) + 2 |m| |dm| = u (2 + 2 |m r| + 6 (m r)^2) / r^2, so r by half of that,
      relatively, plus its own rounding: (2 + |m r| + 3 (m r)^2) u, times |(x_i - m) r d_i|;
    - 60 > 53 + 1 + 2 leaves room for the fp64 steps (below 2^-40 relative here).
    A sorted row moves by at most the largest element error and so does a mean of absolute differences of two sorted rows by the sum of
    the two sets' errors: |swd_device - swd_fp64| <= 1e3 * (bound_a + bound_b) <= 2e3 * this."""
    u = 2.0 ** -24
    out = np.zeros(L)
    for lap in (pyramid(a, L)[1], pyramid(b, L)[1]):
        for l in range(L):
            d = descriptors(lap[l], pos[:, l])
            _, _, mean, rstd = stats(d)
            mr = np.abs(mean) * rstd
            x = np.abs(d).reshape(-1, 3, 49)
            first = ((60 + mr + 3 * mr * mr) * rstd)[None, :, None] * (x + np.abs(mean)[None, :, None])
            for r in range(dirs.shape[0]):
                ad = np.abs(dirs[r].astype(np.float64)).reshape(-1, 3, 49)
                e = u * (np.einsum("mck,dck->md", first, ad) + 2 * np.einsum("c,dck->d", 1 + mr, ad)[None, :])
                out[l] = max(out[l], float(e.max()))
    return out


def pictures(n, S, seed):
    """n uint8 pictures: random bytes, all 0, all 255, a one-pixel checkerboard, then smooth random ones"""
    g = np.random.default_rng(seed)
    x = g.integers(0, 256, size=(n, S, S, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:S, 0:S]
    kinds = [None, np.zeros((S, S, 3), np.uint8), np.full((S, S, 3), 255, np.uint8), np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)]
    for i in range(1, min(n, 4)):
        x[i] = kinds[i]
    for i in range(4, n):
        t = np.linspace(0, 3.0, S)
        wave = np.sin(t[:, None] * g.uniform(0.5, 3) + g.uniform(0, 6)) * np.cos(t[None, :] * g.uniform(0.5, 3) + g.uniform(0, 6))
        x[i] = np.clip(128 + 90 * wave[:, :, None] * g.uniform(0.3, 1, 3) + g.normal(0, 12, (S, S, 3)), 0, 255).astype(np.uint8)
    return x


def corners(n, S, L, P, seed):
    """int32 [n,L,P,2]: random corners, the first four of every picture and level the four extreme ones"""
    g = np.random.default_rng(seed)
    pos = np.zeros((n, L, P, 2), np.int32)
    for l in range(L):
        hi = (S >> l) - 7
        pos[:, l] = g.integers(0, hi + 1, size=(n, P, 2))
        for k, c in enumerate(((0, 0), (hi, hi), (0, hi), (hi, 0))[:P]):
            pos[:, l, k] = c
    return pos


def unit_dirs(R, D, seed):
    d = np.random.default_rng(seed).standard_normal((R, D, 147))
    return (d / np.sqrt((d * d).sum(axis=2, keepdims=True))).astype(np.float32)
