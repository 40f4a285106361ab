"""fp64 restatements of KID and improved precision / recall for tests/test_pairstats_*.py: explicit difference tensors and
explicit i != j masks, nothing shared with the code under test."""
import numpy as np

EPS32 = 2.0 ** -24
MARGIN = 2.5e-5        # 3 * (D + 2) * 2^-24 at D = 128: an upper bound of the fp32 error of d2 relative to |a|^2 + |b|^2


def recipe(D, seed=0):
    g = np.random.default_rng(seed)
    real = g.standard_normal((333, D))
    fake = 0.8 * g.standard_normal((131, D)) + 0.3
    return real.astype(np.float32), fake.astype(np.float32)


def int_features(n, D=64, seed=0):
    return np.random.default_rng(seed).integers(-3, 4, size=(n, D)).astype(np.float32)


def poly3_ref(x, y, skip_diag=False, gamma=None, coef0=1.0):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    with np.errstate(all="ignore"):
        v = (gamma * (x @ y.T) + coef0) ** 3
    keep = np.ones(v.shape, bool)
    if skip_diag:
        keep = np.arange(x.shape[0])[:, None] != np.arange(y.shape[0])[None, :]
    return float(v[keep].sum())


def kid_ref(real, fake):
    m, n = real.shape[0], fake.shape[0]
    return poly3_ref(real, real, True) / (m * (m - 1)) + poly3_ref(fake, fake, True) / (n * (n - 1)) - 2 * poly3_ref(real, fake) / (m * n)


def _sum_bound(a, b, skip_diag):
    """what one normalised kernel sum may differ by when the dot product is a D-term fp32 fmaf chain (error <= (D+2) 2^-24 sum|a_c b_c|)
    and the cube, in fp64, magnifies a relative error by 3"""
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    D = a.shape[1]
    v = (a @ b.T / D + 1.0) ** 3
    keep = np.ones(v.shape, bool)
    if skip_diag:
        keep = np.arange(a.shape[0])[:, None] != np.arange(b.shape[0])[None, :]
    return 3 * (D + 2) * EPS32 * float(v[keep].mean())


def kid_tol(real, fake):
    return _sum_bound(real, real, True) + _sum_bound(fake, fake, True) + 2 * _sum_bound(real, fake, False)


def d2_ref(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([((a[i:i + 64, None, :] - b[None, :, :]) ** 2).sum(axis=-1) for i in range(0, len(a), 64)])      # 64 rows at a time


def radii_ref(x, k):
    d2 = d2_ref(x, x)
    d2[np.arange(len(x)), np.arange(len(x))] = np.inf           # i != j by index: a duplicate row stays a neighbour
    return np.sort(d2, axis=1)[:, k - 1]


def hits_ref(q, ref, r2):
    return (d2_ref(q, ref) <= np.asarray(r2, np.float64)[None, :]).any(axis=1)


def pr_ref(real, fake, k=3):
    return float(hits_ref(fake, real, radii_ref(real, k)).mean()), float(hits_ref(real, fake, radii_ref(fake, k)).mean())


def margins(q, ref, r2):
    """per query: min_j |d2 - r2_j| / (|q|^2 + |ref_j|^2)"""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    scale = (q * q).sum(1)[:, None] + (ref * ref).sum(1)[None, :]
    return (np.abs(d2_ref(q, ref) - np.asarray(r2, np.float64)[None, :]) / scale).min(axis=1)


def radii_bound(x):
    """the k-th smallest of perturbed distances moves by at most the largest perturbation: MARGIN * (|x_i|^2 + max_j |x_j|^2)"""
    n2 = (np.asarray(x, np.float64) ** 2).sum(1)
    return MARGIN * (n2 + n2.max())
