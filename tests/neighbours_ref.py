"""fp64 / int64 restatement of the nearest-neighbour index search for tests/test_neighbours_*.py: explicit difference tensors, a
stable sort by (d2, index), nothing shared with the code under test."""
import numpy as np

from pairstats_ref import EPS32

KMAX = 8


def full_d2(q, ref):
    """[M,N] fp64 squared distances from differences, a few million elements of the difference tensor at a time"""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    rows = max(1, (1 << 22) // (ref.shape[0] * ref.shape[1]))
    with np.errstate(all="ignore"):
        return np.concatenate([((q[i:i + rows, None, :] - ref[None, :, :]) ** 2).sum(axis=-1) for i in range(0, len(q), rows)])


def eligible_d2(q, ref, q_base=0, ref_base=0, exclude_self=False):
    """full_d2 with +inf where a pair is no candidate: a non-finite reference row, and with exclude_self the pair of equal global
    indices"""
    d2 = full_d2(q, ref)
    with np.errstate(all="ignore"):
        d2[:, ~np.isfinite((np.asarray(ref, np.float64) ** 2).sum(1))] = np.inf
    d2[np.isnan(d2)] = np.inf
    if exclude_self:
        gi = q_base + np.arange(len(q))[:, None]
        gj = ref_base + np.arange(len(ref))[None, :]
        d2[gi == gj] = np.inf
    return d2


def knn_ref(q, ref, k, q_base=0, ref_base=0, exclude_self=False):
    """(idx int64 [M,k], d2 fp64 [M,k]): ascending by (d2, index) - a stable sort over indices in order; tail -1 / +inf; a non-finite
    query row -1 / NaN"""
    d2 = eligible_d2(q, ref, q_base, ref_base, exclude_self)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    d = np.take_along_axis(d2, order, axis=1)
    idx = np.where(d < np.inf, ref_base + order, -1).astype(np.int64)
    if idx.shape[1] < k:
        pad = k - idx.shape[1]
        idx = np.concatenate([idx, np.full((len(idx), pad), -1, np.int64)], axis=1)
        d = np.concatenate([d, np.full((len(d), pad), np.inf)], axis=1)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite((np.asarray(q, np.float64) ** 2).sum(1))
    idx[bad], d[bad] = -1, np.nan
    return idx, d


def merge_ref(parts, k):
    """the (idx, d2) results of several reference chunks -> the k smallest by (d2, idx), padding entries (-1) last"""
    idx, d = np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
    key = np.where(idx < 0, np.iinfo(np.int64).max, idx)
    order = np.lexsort((key, d), axis=1)[:, :k]
    return np.take_along_axis(idx, order, axis=1), np.take_along_axis(d, order, axis=1)


def decidable(q, ref, q_base=0, exclude_self=False):
    """bool [M]: the queries whose first 8 neighbours an fp32 two-stage search must reproduce.  With the sorted fp64 distances
    s_0 <= s_1 <= ...:  (a) the candidate cut: s_8 - s_7 > 2 * 3 (D + 2) 2^-24 (|q|^2 + max |ref|^2), twice the bound of the fp32 Gram
    distance's error; (b) the ranks: s_{t+1} - s_t > 2 (D + 4) 2^-24 s_{t+1} for t = 0..7, twice the bound of the difference sum's."""
    q64, r64 = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    D = q64.shape[1]
    s = np.sort(eligible_d2(q, ref, q_base, 0, exclude_self), axis=1)[:, :KMAX + 1]
    ok = np.ones(len(q64), bool)
    if s.shape[1] > KMAX:
        scale = (q64 * q64).sum(1) + (r64 * r64).sum(1).max()
        ok &= (s[:, KMAX] - s[:, KMAX - 1]) > 2 * 3 * (D + 2) * EPS32 * scale
    ok &= ((s[:, 1:] - s[:, :-1]) > 2 * (D + 4) * EPS32 * s[:, 1:]).all(axis=1)
    return ok


def pair_d2(q, ref, idx, ref_base=0):
    """fp64 distance of every pair (i, idx[i][t]) that a result names; NaN where idx is -1"""
    q64, r64 = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    j = np.where(idx >= 0, idx - ref_base, 0)
    d = ((q64[:, None, :] - r64[j]) ** 2).sum(axis=2)
    return np.where(idx >= 0, d, np.nan)


def gram_d2(q, ref):
    """[M,N] fp64 squared distances from the Gram form, for references too large for a difference tensor.  Its ABSOLUTE error is about
    (D + 2) 2^-53 (|q|^2 + |ref|^2) - 1e-11 at D = 12 288 with entries in [-1, 1] - so it ranks and bounds distances of order 1e-2 and
    above with digits to spare; pair_d2 gives the distances of named pairs from differences."""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    return np.maximum(((q * q).sum(1)[:, None] + (ref * ref).sum(1)[None, :]) - 2.0 * (q @ ref.T), 0.0)
