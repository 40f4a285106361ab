"""k-means over feature rows and mode coverage from the cluster histograms: did the generator collapse, and which modes are missing?

    r = kmeans(rows, 100)                              # rows: fp32 [N,D], a CUDA tensor (device) or a numpy array (host)
    r["centres"], r["labels"], r["count"]              # k-means++ seeding, Lloyd iterations, deterministic for a seed
    c = coverage(r["count"], sample_labels)            # c["covered"], c["expected_covered"], c["kl"], c["missing"]

The cluster histograms of the training set and of the samples are compared as in VEEGAN (Srivastava et al. 2017) and PacGAN (Lin et al.
2018): the modes covered and the reverse KL divergence KL(samples || train).  The cluster ids are also the usual pseudo-labels of
unlabelled pictures (self-conditioned GANs, Liu et al. 2020).
Both halves of a Lloyd iteration are twins in metrics.py: the assignment is metrics.nearest(x, centres, 1) (jck_knn_index_f32:
distances from differences, ties to the lower index), the update is metrics.segment_mean (jck_segment_mean_f32: no float atomics, the
bits of a cluster's sum depend only on its own rows in ascending index).  A CUDA tensor runs both on the device, anything else in
numpy - so the loop below has one form, and on exactly representable data the two give the same bits."""
import numpy as np
import torch

from ._lib import JckError

K_MAX = 1024                                           # jck_segment_mean_f32's limit


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _seed_rows(x, k, seed, nearest, on_dev):
    """k-means++ (Arthur & Vassilvitskii 2007), defined completely: u = default_rng(seed).random(k) in fp64; the first centre is row
    int(u[0] * N); centre t is the first row whose running sum of d2min (the squared distance to the nearest centre so far, summed in
    fp64 in row order) exceeds u[t] times the total; a total of 0 (every row is a centre's copy) picks the lowest row not picked yet."""
    n = x.shape[0]
    u = np.random.default_rng(int(seed)).random(k)
    picked = [min(n - 1, int(u[0] * n))]
    d2min = None
    for t in range(1, k):
        d2 = nearest(x, x[picked[-1]:picked[-1] + 1], 1)[1][:, 0]
        if on_dev:
            d2min = d2 if d2min is None else torch.minimum(d2min, d2)
            if t == 1 and bool(torch.isnan(d2min).any()):
                raise JckError("kmeans: a row of x is not finite")
            cum = torch.cumsum(d2min.double(), 0)
            total = float(cum[-1])
            row = int(torch.searchsorted(cum, torch.tensor([u[t] * total], dtype=torch.float64, device=cum.device), right=True)[0]) if total > 0 else -1
        else:
            d2min = d2 if d2min is None else np.minimum(d2min, d2)
            if t == 1 and np.isnan(d2min).any():
                raise JckError("kmeans: a row of x is not finite")
            cum = np.cumsum(d2min.astype(np.float64))
            total = float(cum[-1])
            row = int(np.searchsorted(cum, u[t] * total, side="right")) if total > 0 else -1
        if row < 0:
            taken = set(picked)
            row = next(i for i in range(n) if i not in taken)
        picked.append(min(n - 1, row))
    return picked


def kmeans(x, k, iters=50, seed=0, chunk=None):
    """Lloyd's k-means of the rows of x [N,D] (fp32; a CUDA tensor runs on the device, a numpy array or host tensor in numpy) from a
    k-means++ seeding (_seed_rows) -> {"centres" fp32 [k,D], "labels" int64 [N], "count" int64 [k], "d2" [N] (each row's squared
    distance to its centre), "inertia" float (their fp64 sum), "iters": updates made, "history": the inertia of every assignment}.
    An iteration assigns (metrics.nearest, the centres walked `chunk` rows at a time), stops where the labels are the previous ones,
    else updates (metrics.segment_mean); an empty cluster keeps its centre and reports count 0.  After the last of `iters` updates
    the rows are assigned once more: labels, count and inertia always belong to the centres returned.  A non-finite row: JckError."""
    from metrics import nearest, segment_mean
    on_dev = torch.is_tensor(x) and x.is_cuda
    x = x.detach().to(torch.float32).contiguous() if on_dev else np.ascontiguousarray(_np(x), dtype=np.float32)
    k, iters = int(k), int(iters)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise JckError(f"kmeans: x must be a non-empty [N, D] matrix, got {tuple(x.shape)}")
    if not 1 <= k <= min(K_MAX, x.shape[0]):
        raise JckError(f"kmeans: k = {k} needs 1 <= k <= min({K_MAX}, rows = {x.shape[0]})")
    if iters < 0:
        raise JckError(f"kmeans: iters = {iters} must be >= 0")
    rows = _seed_rows(x, k, seed, nearest, on_dev)
    centres = x[torch.as_tensor(rows, device=x.device)].clone() if on_dev else x[np.asarray(rows)].copy()
    same = torch.equal if on_dev else np.array_equal
    history, done, before = [], 0, None
    while True:
        idx, d2 = nearest(x, centres, 1, chunk=chunk)
        if bool((idx < 0).any()):
            raise JckError("kmeans: a row of x is not finite")
        history.append(float(d2.double().sum()) if on_dev else float(d2.astype(np.float64).sum()))
        if (before is not None and same(idx, before)) or done == iters:
            break
        centres = segment_mean(x, idx, k, centre=centres)[2]
        before, done = idx, done + 1
    labels = idx[:, 0]
    count = torch.bincount(labels, minlength=k) if on_dev else np.bincount(labels, minlength=k).astype(np.int64)
    return {"centres": centres, "labels": labels, "count": count, "d2": d2[:, 0], "inertia": history[-1], "iters": done, "history": history}


def coverage(count_real, labels_fake, min_count=1):
    """Mode coverage of samples against a clustered training set, on the host in fp64.  count_real [k]: the training set's cluster
    sizes (kmeans' "count"); labels_fake [n]: the samples' clusters.  Clusters without a real member are dropped from everything,
    the samples that landed in them too (labels outside 0..k-1 as well) ->
      k, k_real          clusters in all / with a real member
      hist_real, hist_fake   int64 [k] counts per cluster id (0 in both at a dropped cluster)
      covered            clusters with hist_fake >= min_count
      expected_covered   sum_c 1 - (1 - p_c)^n at the real proportions p_c and n samples: what a perfect generator reaches at min_count
                         = 1, so that a small n is not read as collapse
      kl                 sum_c q_c ln(q_c / p_c) over q_c > 0, in nats: q the samples' proportions (NaN without samples)
      missing            int64: the uncovered cluster ids, largest real share first (ties: the lower id)"""
    real = np.asarray(_np(count_real)).astype(np.int64).reshape(-1)
    lab = np.asarray(_np(labels_fake)).astype(np.int64).reshape(-1)
    k, min_count = real.shape[0], int(min_count)
    if k < 1 or (real < 0).any() or real.sum() < 1:
        raise JckError("coverage: count_real must hold k >= 1 cluster sizes >= 0, one of them positive")
    if min_count < 1:
        raise JckError(f"coverage: min_count = {min_count} must be >= 1")
    keep = real > 0
    fake = np.bincount(lab[(lab >= 0) & (lab < k)], minlength=k).astype(np.int64)
    fake[~keep] = 0
    n = int(fake.sum())
    p = real[keep] / float(real.sum())
    hit = fake[keep] >= min_count
    ids = np.flatnonzero(keep)
    gone = ids[~hit]
    missing = gone[np.argsort(-real[gone], kind="stable")]
    kl = float("nan")
    if n > 0:
        q = fake[keep] / float(n)
        kl = float((q[q > 0] * np.log(q[q > 0] / p[q > 0])).sum())
    return {"k": k, "k_real": int(keep.sum()), "covered": int(hit.sum()), "expected_covered": float((1.0 - (1.0 - p) ** n).sum()), "kl": kl,
            "hist_real": np.where(keep, real, 0), "hist_fake": fake, "missing": missing.astype(np.int64)}
