"""fp64 restatement of the power spectra of pictures, written from the definition and sharing no code with
metrics.spectrum or hipgan.spectrum: the transform is F = D X D^T with the DFT matrix built from (k j) mod S (angles reduced exactly, no
np.fft), the bin rule is a search in integers, and bound(S) is the derived error bound B(S) of csrc/spectrum.hip.

B(S).  u = 2^-24.  A radix-2 Cooley-Tukey transform of t stages whose twiddles are accurate to mu satisfies ||F^ - F||_2 <= e ||F||_2
with e = t eta / (1 - t eta), eta = mu + gamma_4 (sqrt 2 + mu), gamma_4 = 4u / (1 - 4u) (Higham, Accuracy and Stability of Numerical
Algorithms, Th. 24.2); twiddles rounded from fp64 have mu = u.  The kernel runs log2 S stages along the rows and log2 S down the
columns: t = 2 log2 S.  Its real-input split (two rows per complex transform) is an isometry followed by one rounding per component: a
factor (1 + u).  The input carries at most three roundings (the conversion of the centred integer, two window products):
e_in = (1 + u)^3 - 1.  So e = e_in + (1 + e_in)((1 + e_fft)(1 + u) - 1), and by Cauchy-Schwarz sum |P^ - P| <= (2 e + e^2) E with E the sum
of the exact P.  The fp64 steps (power, bin sums, partial planes of fewer than 2^13 terms) add 2^-40.  B(32), B(64), B(128) = 8.41e-6,
1.000e-5, 1.159e-5; the cap on B(128) is 2e-5."""
import numpy as np

LUMA = (77, 150, 29)
U = 2.0 ** -24


def bound(S):
    t = 2 * (int(S).bit_length() - 1)
    mu = U
    g4 = 4 * U / (1 - 4 * U)
    eta = mu + g4 * (np.sqrt(2.0) + mu)
    e_fft = t * eta / (1 - t * eta)
    e_in = (1 + U) ** 3 - 1
    e = e_in + (1 + e_in) * ((1 + e_fft) * (1 + U) - 1)
    return float((2 * e + e * e) * (1 + 2.0 ** -40) + 2.0 ** -40)


def bin_of(d2):
    """the unique integer r with r^2 - r < d2 <= r^2 + r (0 at d2 = 0), found by counting up in integers"""
    r = 0
    while r * r + r < d2:
        r += 1
    return r


def bin_map(S):
    out = np.zeros((S, S), dtype=np.int64)
    for u in range(S):
        for v in range(S):
            out[u, v] = bin_of(min(u, S - u) ** 2 + min(v, S - v) ** 2)
    return out


def dft_matrix(S):
    """D[k][j] = exp(-2 pi i ((k j) mod S) / S): the product is reduced in integers, and the four axis angles are exact"""
    kj = (np.arange(S)[:, None] * np.arange(S)[None, :]) % S
    ang = 2.0 * np.pi * kj.astype(np.float64) / S
    c, s = np.cos(ang), np.sin(ang)
    for q, (cv, sv) in enumerate(((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))):
        at = kj * 4 == q * S
        c[at], s[at] = cv, sv
    return c - 1j * s


def hann32(S):
    return np.array([0.5 - 0.5 * np.cos(2.0 * np.pi * j / S) for j in range(S)], dtype=np.float64).astype(np.float32)


def plane_int(x, plane):
    """the integer Y of the definition, int64 [n,S,S]"""
    x = x.astype(np.int64)
    if plane in (3, "luma"):
        return LUMA[0] * x[..., 0] + LUMA[1] * x[..., 1] + LUMA[2] * x[..., 2]
    return 256 * x[..., {"r": 0, "g": 1, "b": 2}.get(plane, plane)]


def power(x, plane, window):
    """uint8 [n,S,S,3] -> (P fp64 [n][S][S], mean fp64 [n])"""
    Y = plane_int(x, plane)
    n, S = Y.shape[0], Y.shape[1]
    D = dft_matrix(S)
    P, mean = np.zeros((n, S, S)), np.zeros(n)
    W = 1.0
    w = None
    if window == "hann":
        w = hann32(S).astype(np.float64)
        W = float((w * w).sum() / S) ** 2
    for i in range(n):
        T = int(Y[i].sum())
        mean[i] = T / (256.0 * S * S)
        val = (S * S * Y[i] - T).astype(np.float64) / (256.0 * S * S)
        if w is not None:
            val = (val * w[:, None]) * w[None, :]
        F = D @ val @ D.T
        P[i] = (F.real ** 2 + F.imag ** 2) / (S * S * W)
    return P, mean


def profile(P):
    """fp64 [n][S][S] -> (prof [n][R], count [R])"""
    n, S = P.shape[0], P.shape[1]
    b = bin_map(S)
    R = int(b.max()) + 1
    count = np.array([(b == r).sum() for r in range(R)], dtype=np.int64)
    prof = np.array([[P[i][b == r].sum() / count[r] for r in range(R)] for i in range(n)]).reshape(n, R)
    return prof, count


def pictures(n, S, seed):
    """uint8 [n,S,S,3], in this order (cycled): random bytes, all 0, all 255, a one-pixel checkerboard of 0 / 255, one bright pixel on
    black, a byte-quantised cosine at an integer frequency along x, a smooth picture plus unit noise"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    out = np.zeros((n, S, S, 3), dtype=np.uint8)
    for i in range(n):
        kind = i % 7
        if kind == 0:
            out[i] = g.integers(0, 256, size=(S, S, 3))
        elif kind == 1:
            out[i] = 0
        elif kind == 2:
            out[i] = 255
        elif kind == 3:
            out[i] = (255 * ((yy + xx) & 1))[:, :, None]
        elif kind == 4:
            out[i, int(g.integers(0, S)), int(g.integers(0, S))] = (255, 200, 90)
        elif kind == 5:
            f = int(g.integers(1, S // 2))
            wave = np.rint(127.5 + 100.0 * np.cos(2.0 * np.pi * f * xx / S))
            out[i] = np.clip(wave[:, :, None] + np.array([0, 10, -10])[None, None, :], 0, 255)
        else:
            smooth = 128 + 60 * np.sin(2 * np.pi * yy / S + 0.3)[:, :, None] * np.cos(2 * np.pi * xx[:, :, None] / S + np.array([0.0, 0.7, 1.9])[None, None, :])
            out[i] = np.clip(np.rint(smooth + g.integers(-1, 2, size=(S, S, 3))), 0, 255)
    return out
