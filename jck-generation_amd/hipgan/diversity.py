"""Sample diversity from the structural similarity of random pairs: does every sample of a class look the same?

    pr = draw_pairs(n, 1000, seed=0, groups=class_ids)         # random pairs inside every class
    r = metrics.ssim_pairs(u8, u8, pr["i"], pr["j"])           # SSIM / MS-SSIM per pair (csrc/ssim.hip on CUDA tensors, numpy else)
    s = summarise(r["ms_ssim"], pr["group"])                   # mean, standard error, n - overall and per class
    c = compare(s, summarise(train_values, train_groups))      # per class: are the samples less diverse than the training pictures?

The mean MS-SSIM between random pairs of samples of a class, beside the same number for the training pictures of that class, is the
diversity measure of AC-GAN (Odena et al. 2017, section 4.3): a class whose samples are more similar to each other than its training
pictures are has (partly) collapsed.  The helpers here are host code in fp64; the pair kernel and its numpy twin are
metrics.ssim_pairs."""
import numpy as np
import torch

from ._lib import JckError


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def max_levels(S):
    """the largest admissible L of metrics.ssim_pairs at S: S % 2^(L-1) == 0 and S >> (L-1) >= 11, at most 4; 0 when S is outside 11..128
    (jck_ssim_max_levels gives the same)"""
    S = int(S)
    if not 11 <= S <= 128:
        return 0
    L = 1
    while L < 4 and S % (1 << L) == 0 and (S >> L) >= 11:
        L += 1
    return L


def default_levels(S):
    """the largest admissible L with S >> (L-1) >= 16 (32 -> 2, 64 -> 3, 128 -> 4), 1 if there is none"""
    return max([L for L in range(1, max_levels(S) + 1) if (int(S) >> (L - 1)) >= 16], default=1)


def _pairs_of(n, p, rng):
    """p pairs i != j of 0..n-1 from rng, or every pair i < j in lexicographic order when p >= n (n - 1) / 2"""
    if p >= n * (n - 1) // 2:
        i, j = np.triu_indices(n, 1)
        return i.astype(np.int64), j.astype(np.int64)
    i = rng.integers(0, n, p)
    j = rng.integers(0, n - 1, p)
    j += j >= i
    return i.astype(np.int64), j.astype(np.int64)


def draw_pairs(n, p, seed, groups=None):
    """Pairs of distinct indices of 0..n-1 -> {"i", "j" int64 [P], "group" int64 [P] or None, "dropped": [class ids]}.  Defined
    completely by rng = np.random.default_rng(seed): i = rng.integers(0, n, p), j = rng.integers(0, n - 1, p), j += j >= i; when
    p >= n (n - 1) / 2 every pair i < j in lexicographic order instead (nothing is drawn).  groups (class ids [n]): the same inside
    each class's member list (ascending indices), p per class from the ONE rng, classes ascending; a class with fewer than two
    members has no pair and is listed in "dropped"."""
    n, p = int(n), int(p)
    if p < 1:
        raise JckError(f"draw_pairs: p = {p} must be >= 1")
    rng = np.random.default_rng(int(seed))
    if groups is None:
        if n < 2:
            raise JckError(f"draw_pairs: n = {n} must be >= 2")
        i, j = _pairs_of(n, p, rng)
        return {"i": i, "j": j, "group": None, "dropped": []}
    g = _np(groups).astype(np.int64).reshape(-1)
    if g.shape[0] != n:
        raise JckError(f"draw_pairs: {g.shape[0]} group ids for n = {n}")
    ii, jj, gg, dropped = [], [], [], []
    for c in np.unique(g):
        members = np.flatnonzero(g == c)
        if members.shape[0] < 2:
            dropped.append(int(c))
            continue
        i, j = _pairs_of(members.shape[0], p, rng)
        ii.append(members[i]); jj.append(members[j]); gg.append(np.full(i.shape[0], c, np.int64))
    if not ii:
        raise JckError("draw_pairs: no class has two members")
    return {"i": np.concatenate(ii), "j": np.concatenate(jj), "group": np.concatenate(gg), "dropped": dropped}


def _stats(v):
    n = int(v.shape[0])
    return {"mean": float(v.mean()) if n else float("nan"), "sem": float(v.std(ddof=1) / np.sqrt(n)) if n > 1 else float("nan"), "n": n}


def summarise(values, groups=None):
    """{"mean", "sem" (the standard error, ddof 1; NaN below two values), "n", "per_class": {class id: the same three}} of per-pair
    values (host or device) in fp64; per_class is empty without groups"""
    v = _np(values).astype(np.float64).reshape(-1)
    out = _stats(v)
    out["per_class"] = {}
    if groups is not None:
        g = _np(groups).astype(np.int64).reshape(-1)
        if g.shape[0] != v.shape[0]:
            raise JckError(f"summarise: {g.shape[0]} group ids for {v.shape[0]} values")
        out["per_class"] = {int(c): _stats(v[g == c]) for c in np.unique(g)}
    return out


def compare(sample_summary, train_summary):
    """Samples against training pictures, from two summarise() results of a similarity: {"overall": sample mean > train mean,
    "per_class": {class id: {"sample", "train", "less_diverse" = sample mean > train mean}} over the classes both have,
    "flagged": the less diverse class ids, "share_less_diverse": their share (NaN without a common class)}"""
    s, t = sample_summary["per_class"], train_summary["per_class"]
    per = {c: {"sample": s[c]["mean"], "train": t[c]["mean"], "less_diverse": bool(s[c]["mean"] > t[c]["mean"])} for c in sorted(set(s) & set(t))}
    flagged = [c for c in per if per[c]["less_diverse"]]
    return {"overall": bool(sample_summary["mean"] > train_summary["mean"]), "per_class": per, "flagged": flagged,
            "share_less_diverse": len(flagged) / len(per) if per else float("nan")}


def top_pairs(ms_ssim, top):
    """the indices of the `top` pairs with the highest MS-SSIM, highest first; ties go to the lower pair index, NaN last"""
    v = _np(ms_ssim).astype(np.float64).reshape(-1)
    return np.argsort(np.where(np.isnan(v), np.inf, -v), kind="stable")[:max(0, int(top))].astype(np.int64)


def pair_diversity(u8, pairs, seed, class_ids=None, levels=None):
    """draw_pairs + metrics.ssim_pairs + summarise on one set of uint8 pictures [n,S,S,3] (device or host; class_ids None: one class 0)
    -> {"pairs", "ssim", "ms_ssim", "sq_err" (host arrays), "summary": {"ms_ssim", "ssim"}, "dropped"}"""
    from metrics import ssim_pairs
    n = int(u8.shape[0])
    pr = draw_pairs(n, pairs, seed, np.zeros(n, np.int64) if class_ids is None else class_ids)
    r = ssim_pairs(u8, u8, pr["i"], pr["j"], levels=levels)
    out = {key: _np(r[key]) for key in ("ssim", "ms_ssim", "sq_err")}
    out["pairs"] = pr
    out["dropped"] = pr["dropped"]
    out["summary"] = {key: summarise(out[key], pr["group"]) for key in ("ms_ssim", "ssim")}
    return out
