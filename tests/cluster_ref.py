"""fp64 restatement of the clustering layer (csrc/cluster.hip, metrics.segment_mean, hipgan/cluster.py): per-cluster sums, the k-means++
seeding, Lloyd iterations and the coverage figures, written as plain loops over exact distances - nothing here calls the code under test."""
import numpy as np

U32 = 2.0 ** -24                                      # fp32 unit roundoff


def segment_ref(x, labels, k, centre=None):
    """(sum fp64 [k,D], count int64 [k], centre fp32 [k,D]): rows with labels outside 0..k-1 skipped; centre = fp32(sum) / fp32(count)
    in fp32 where count > 0, the given row (zeros without one) elsewhere"""
    x, labels = np.asarray(x, np.float64), np.asarray(labels).reshape(-1)
    total, count = np.zeros((k, x.shape[1])), np.zeros(k, np.int64)
    for i, c in enumerate(labels):
        if 0 <= c < k:
            total[c] += x[i]
            count[c] += 1
    out = np.zeros((k, x.shape[1]), np.float32) if centre is None else np.array(centre, dtype=np.float32)
    for c in range(k):
        if count[c]:
            out[c] = total[c].astype(np.float32) / np.float32(count[c])
    return total, count, out


def d2_ref(x, centres):
    """exact squared distances [N,k] in fp64 from differences"""
    x, centres = np.asarray(x, np.float64), np.asarray(centres, np.float64)
    return ((x[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)


def seed_ref(x, k, seed):
    """the rows k-means++ picks, as hipgan.cluster defines it"""
    n = x.shape[0]
    u = np.random.default_rng(seed).random(k)
    picked = [int(u[0] * n)]
    d2min = np.full(n, np.inf)
    for t in range(1, k):
        d2min = np.minimum(d2min, d2_ref(x, x[picked[-1]:picked[-1] + 1])[:, 0])
        cum = np.cumsum(d2min)
        if cum[-1] == 0:
            picked.append(min(set(range(n)) - set(picked)))
        else:
            picked.append(int(np.argmax(cum > u[t] * cum[-1])))
    return picked


def assign_ref(x, centres):
    d2 = d2_ref(x, centres)
    labels = d2.argmin(axis=1)                        # the first minimum: ties to the lower index
    return labels.astype(np.int64), d2[np.arange(x.shape[0]), labels]


def kmeans_ref(x, k, iters=50, seed=0):
    x = np.asarray(x, np.float32)
    centres = x[seed_ref(x, k, seed)].copy()
    history, done, before = [], 0, None
    while True:
        labels, d2 = assign_ref(x, centres)
        history.append(float(d2.sum()))
        if (before is not None and np.array_equal(labels, before)) or done == iters:
            break
        centres = segment_ref(x, labels, k, centres)[2]
        before, done = labels, done + 1
    return {"centres": centres, "labels": labels, "count": np.bincount(labels, minlength=k).astype(np.int64), "inertia": history[-1],
            "iters": done, "history": history}


def coverage_ref(count_real, labels_fake, min_count=1):
    real = [int(v) for v in count_real]
    k = len(real)
    fake = [0] * k
    for c in labels_fake:
        if 0 <= c < k and real[c] > 0:
            fake[int(c)] += 1
    n, total = sum(fake), sum(real)
    ids = [c for c in range(k) if real[c] > 0]
    kl = sum(fake[c] / n * np.log((fake[c] / n) / (real[c] / total)) for c in ids if fake[c] > 0)
    missing = sorted((c for c in ids if fake[c] < min_count), key=lambda c: (-real[c], c))
    return {"k": k, "k_real": len(ids), "covered": sum(1 for c in ids if fake[c] >= min_count),
            "expected_covered": sum(1.0 - (1.0 - real[c] / total) ** n for c in ids), "kl": float(kl), "hist_real": real, "hist_fake": fake,
            "missing": missing}


def blobs(seed=0, n_blobs=6, per=40, D=8, spread=3):
    """6 blobs of 40 integer rows: centres on multiples of 16 (distinct), integer spread -spread..spread, shuffled -> (x fp32, blob id)"""
    g = np.random.default_rng(seed)
    centres = set()
    while len(centres) < n_blobs:
        centres.add(tuple(int(v) for v in g.integers(-4, 5, size=D) * 16))
    centres = np.array(sorted(centres), np.float32)
    which = np.repeat(np.arange(n_blobs), per)
    x = centres[which] + g.integers(-spread, spread + 1, size=(n_blobs * per, D)).astype(np.float32)
    order = g.permutation(x.shape[0])
    return x[order].astype(np.float32), which[order]
