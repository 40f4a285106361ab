"""Inception-Score / FID / intra-FID with the reference's interface (metrics.py:19-141): `Metrics(real_images)`,
`.inception_score(loader, splits=10)`, `.fid(loader, intra_fid=False, label=0)`, `.intra_fid(tensor)`.

The arithmetic is the reference's (100-d logits of a CIFAR-100 fine-tuned Inception-v3, softmax/KL per split, mean/cov +
scipy sqrtm, 20 superclass FIDs summed and divided by 100).  The feature extractor is pluggable; by default it is the
reference's network (inception_v3 with a Linear(2048,100) head, weights from ./save/iception_v3/loss_bset.pt, metrics.py:
46-51) run by the hand-written HIP chain of `inception.InceptionV3Hip` - no torchvision needed; when the weights file is
missing, construction raises MetricsUnavailable and the trainer carries on without scores.  Feature means and covariances are
formed in fp64 on the device (jck_mean_cov_f64) when the features live there; the matrix square root stays on the host
(scipy), as in the reference.  Beyond the reference (opt-in in the trainers): KID, intra-KID and improved precision / recall
from pairwise kernels over the feature matrices (csrc/pairstat.hip; numpy fp64 for host arrays), and the nearest real rows of
given rows with their indices (csrc/knnindex.hip), and per-cluster sums and means of rows (csrc/cluster.hip; with `nearest` the two
halves of a k-means iteration, hipgan/cluster.py).  Fixes the reference's `.targets` defect for DCGAN (its loader has none): targets are optional."""
import os
import pickle

import numpy as np
import torch
from scipy.linalg import sqrtm

from utils import get_default_device

SUPERCLASS_MEMBERS = (
    (4, 30, 55, 72, 95), (1, 32, 67, 73, 91), (54, 62, 70, 82, 92), (9, 10, 16, 28, 61), (0, 51, 53, 57, 83),
    (22, 39, 40, 86, 87), (5, 20, 25, 84, 94), (6, 7, 14, 18, 24), (3, 42, 43, 88, 97), (12, 17, 37, 68, 76),
    (23, 33, 49, 60, 71), (15, 19, 21, 31, 38), (34, 63, 64, 66, 75), (26, 45, 77, 79, 99), (2, 11, 35, 46, 98),
    (27, 29, 44, 78, 93), (36, 50, 65, 74, 80), (47, 52, 56, 59, 96), (8, 13, 48, 58, 90), (41, 69, 81, 85, 89))


class MetricsUnavailable(RuntimeError):
    pass


def default_extractor(device, weights="./save/iception_v3/loss_bset.pt"):
    """The reference's metric network from a LOCAL weights file (torchvision key names), on the HIP kernels."""
    if not os.path.exists(weights):
        raise MetricsUnavailable(f"fine-tuned Inception weights not found at {weights} (the reference loads them at metrics.py:51; "
                                 f"they are not part of its repository)")
    if not torch.cuda.is_available():
        raise MetricsUnavailable("the metric network runs on the GPU (no CPU fallback)")
    from inception import InceptionV3Hip
    return InceptionV3Hip.from_file(weights, device)


def mean_cov_device(x):
    """(mean [D], covariance [D,D]) of a CUDA tensor as fp64 DEVICE tensors (jck_mean_cov_f64; no host sync)."""
    from hipgan._lib import cur_stream, lib
    x = x.to(torch.float32).contiguous()
    n, d = x.shape
    mu = torch.empty(d, dtype=torch.float64, device=x.device)
    cov = torch.empty(d, d, dtype=torch.float64, device=x.device)
    lib.jck_mean_cov_f64(x, mu, cov, n, d, cur_stream())
    return mu, cov


def mean_cov(x):
    """(mean [D], covariance [D,D]) in float64 as np.mean(axis=0) / np.cov(rowvar=False) give them (metrics.py:120-126).  A
    CUDA tensor is reduced on the device (fp64 accumulation, fixed summation order); anything else by numpy."""
    if torch.is_tensor(x) and x.is_cuda:
        mu, cov = mean_cov_device(x)
        return mu.cpu().numpy(), cov.cpu().numpy()
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.mean(x, axis=0), np.cov(x, rowvar=False)


def fid_from_stats(mu1, sigma1, mu2, sigma2):
    """reference metrics.py:127-129 from the two Gaussians' parameters.  Non-finite statistics (a NaN or infinite feature)
    give NaN: scipy's sqrtm refuses such a matrix with a ValueError, which would end the run the score is reported to."""
    mu1, sigma1, mu2, sigma2 = (np.asarray(v, dtype=np.float64) for v in (mu1, sigma1, mu2, sigma2))
    if not all(np.isfinite(v).all() for v in (mu1, sigma1, mu2, sigma2)):
        return float("nan")
    covmean = sqrtm(sigma1.dot(sigma2))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return float(np.sum((mu1 - mu2) ** 2.0) + np.trace(sigma1 + sigma2 - 2.0 * covmean))


def fid_from_features(real, fake):
    """Frechet distance between the Gaussians fitted to two feature matrices (reference metrics.py:120-129)."""
    return fid_from_stats(*mean_cov(real), *mean_cov(fake))


def inception_score_from_probs(preds, splits=10):
    """exp(mean KL(p(y|x) || p(y))) per split, averaged (reference metrics.py:97-110; scipy.stats.entropy semantics)."""
    n = preds.shape[0]
    out = []
    for k in range(splits):
        part = preds[k * (n // splits):(k + 1) * (n // splits), :]
        py = np.mean(part, axis=0)
        pk = part / part.sum(axis=1, keepdims=True)
        qk = py / py.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            kl = np.where(pk > 0, pk * np.log(pk / qk), 0.0).sum(axis=1)
        out.append(np.exp(np.mean(kl)))
    return float(np.mean(out))


# ---- KID and improved precision / recall: pairwise statistics over feature matrices -------------------------------------
# KID (Binkowski et al. 2018) is the unbiased MMD^2 with k(a, b) = (a.b / D + 1)^3 over the FULL sets: unbiased at any
# sample size, no matrix square root.  Improved precision / recall (Kynkaanniemi et al. 2019): a set's manifold is the union
# of the balls around its points that reach the k-th nearest other point; precision = share of fake points inside real's
# manifold (fidelity), recall = share of real points inside fake's (coverage).  CUDA tensors go through the kernels of
# csrc/pairstat.hip (never an M x N matrix in memory), anything else through blocked numpy fp64 of the same formulas.
_HOST_BLOCK = 2048          # rows per Gram block of the numpy paths: 2048 x 2048 fp64 = 32 MiB, whatever the set sizes


def _np64(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float64)


def _pair_device(*xs):
    """the CUDA device the pairwise statistics run on: that of the first CUDA tensor among xs (None: numpy)"""
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return None


def _dev32(x, device):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float32))
    return x.detach().to(device=device, dtype=torch.float32).contiguous()


def poly3_sum(x, y, skip_diag=False):
    """sum_{i,j} (x_i.y_j / D + 1)^3, without the pairs i == j (by index) when skip_diag.  CUDA: a fp64 device tensor [1]
    (jck_poly3_sum_f64: fp32 dot product, fp64 polynomial and sums, fixed order; no host sync); else a Python float."""
    dev = _pair_device(x, y)
    if dev is not None:
        from hipgan._lib import cur_stream, lib, load_library
        x, y = _dev32(x, dev), _dev32(y, dev)
        (m, d), n = x.shape, y.shape[0]
        out = torch.empty(1, dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, load_library().jck_pairstat_ws_bytes(m, n) // 8), dtype=torch.float64, device=dev)
        lib.jck_poly3_sum_f64(x, m, y, n, d, 1.0 / d, 1.0, int(bool(skip_diag)), out, ws, cur_stream())
        return out
    x, y = _np64(x), _np64(y)
    d, total = x.shape[1], 0.0
    with np.errstate(all="ignore"):
        for i in range(0, x.shape[0], _HOST_BLOCK):
            for j in range(0, y.shape[0], _HOST_BLOCK):
                total += float(((x[i:i + _HOST_BLOCK] @ y[j:j + _HOST_BLOCK].T / d + 1.0) ** 3).sum())
        if skip_diag:
            r = min(x.shape[0], y.shape[0])
            total -= float((((x[:r] * y[:r]).sum(axis=1) / d + 1.0) ** 3).sum())
    return total


def knn_radius2(x, k):
    """r2[i] = the k-th smallest squared distance from x_i to the OTHER rows of x (by index: a duplicate row is a neighbour at
    distance 0); NaN for a non-finite row.  CUDA: float32 device tensor (jck_knn_radius2_f32, 1 <= k <= 8); else float64 numpy."""
    if not 1 <= k < x.shape[0]:
        raise ValueError(f"knn_radius2: k = {k} needs 1 <= k < rows = {x.shape[0]}")
    dev = _pair_device(x)
    if dev is not None:
        from hipgan._lib import cur_stream, lib
        x = _dev32(x, dev)
        r2 = torch.empty(x.shape[0], dtype=torch.float32, device=dev)
        lib.jck_knn_radius2_f32(x, x.shape[0], x.shape[1], k, r2, cur_stream())
        return r2
    x = _np64(x)
    n = x.shape[0]
    r2 = np.empty(n)
    with np.errstate(all="ignore"):
        nrm = (x * x).sum(axis=1)
        step = max(1, min(_HOST_BLOCK, (_HOST_BLOCK * _HOST_BLOCK) // n))
        for i in range(0, n, step):
            d2 = np.maximum((nrm[i:i + step, None] + nrm[None, :]) - 2.0 * (x[i:i + step] @ x.T), 0.0)
            rows = np.arange(d2.shape[0])
            d2[rows, i + rows] = np.inf
            d2[np.isnan(d2)] = np.inf                       # a non-finite row is nobody's neighbour
            r2[i:i + step] = np.partition(d2, k - 1, axis=1)[:, k - 1]
    r2[~np.isfinite(nrm)] = np.nan
    return r2


def manifold_hit(q, ref, r2):
    """hit[i] = 1 when q_i lies within sqrt(r2[j]) of some ref_j (a tie is a hit), else 0; 255 for a non-finite q_i.  uint8:
    a CUDA tensor (jck_manifold_hit_u8) when any argument is one, else numpy."""
    dev = _pair_device(q, ref, r2)
    if dev is not None:
        from hipgan._lib import cur_stream, lib
        q, ref, r2 = _dev32(q, dev), _dev32(ref, dev), _dev32(r2, dev)
        hit = torch.empty(q.shape[0], dtype=torch.uint8, device=dev)
        lib.jck_manifold_hit_u8(q, q.shape[0], ref, r2, ref.shape[0], q.shape[1], hit, cur_stream())
        return hit
    q, ref, r2 = _np64(q), _np64(ref), _np64(r2)
    hit = np.zeros(q.shape[0], dtype=np.uint8)
    with np.errstate(all="ignore"):
        nq, nr = (q * q).sum(axis=1), (ref * ref).sum(axis=1)
        for i in range(0, q.shape[0], _HOST_BLOCK):
            for j in range(0, ref.shape[0], _HOST_BLOCK):
                d2 = np.maximum((nq[i:i + _HOST_BLOCK, None] + nr[None, j:j + _HOST_BLOCK]) - 2.0 * (q[i:i + _HOST_BLOCK] @ ref[j:j + _HOST_BLOCK].T), 0.0)
                hit[i:i + _HOST_BLOCK] |= (d2 <= r2[None, j:j + _HOST_BLOCK]).any(axis=1).astype(np.uint8)
    hit[~np.isfinite(nq)] = 255
    return hit


def nearest(q, ref, k, exclude_self=False, chunk=None):
    """(idx int64 [M,k], d2 [M,k]): the k rows of ref nearest to every row of q, ascending by (d2, index) - equal distances go to the
    lower index.  exclude_self leaves out the pair i == j (by index: a duplicate row elsewhere stays a neighbour at distance 0).
    Fewer than k eligible rows: the tail is idx -1 / d2 +inf; a non-finite query row: idx -1 / d2 NaN; a non-finite reference row is
    never a neighbour.  CUDA (any argument a CUDA tensor): device tensors from jck_knn_index_f32 (1 <= k <= 8; fp32 distances from
    differences, within (D + 4) 2^-24 relative), the reference walked `chunk` rows at a time and merged on the device; else float64 numpy."""
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError(f"nearest: k = {k} needs 1 <= k <= 8")
    if q.ndim != 2 or ref.ndim != 2 or q.shape[1] != ref.shape[1] or q.shape[0] < 1 or ref.shape[0] < 1:
        raise ValueError(f"nearest: q and ref must be non-empty [rows, D] matrices of one D, got {tuple(q.shape)} and {tuple(ref.shape)}")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"nearest: chunk = {chunk} must be >= 1")
    dev = _pair_device(q, ref)
    m, n = q.shape[0], ref.shape[0]
    step = n if chunk is None else min(n, int(chunk))
    if dev is not None:
        q = _dev32(q, dev)
        idx = torch.empty(m, k, dtype=torch.int64, device=dev)
        d2 = torch.empty(m, k, dtype=torch.float32, device=dev)
        for lo in range(0, n, step):
            nearest_chunk(q, _dev32(ref[lo:lo + step], dev), k, idx, d2, ref_base=lo, exclude_self=exclude_self, merge=lo > 0)
        return idx, d2
    q, ref = _np64(q), _np64(ref)
    idx, d2 = np.full((m, k), -1, np.int64), np.full((m, k), np.inf)
    with np.errstate(all="ignore"):
        nq, nr = (q * q).sum(axis=1), (ref * ref).sum(axis=1)
        rows = max(1, min(_HOST_BLOCK, (_HOST_BLOCK * _HOST_BLOCK) // n, (_HOST_BLOCK * _HOST_BLOCK) // (16 * q.shape[1])))
        for i in range(0, m, rows):
            g = np.maximum((nq[i:i + rows, None] + nr[None, :]) - 2.0 * (q[i:i + rows] @ ref.T), 0.0)
            g[:, ~np.isfinite(nr)] = np.inf
            g[np.isnan(g)] = np.inf
            if exclude_self:
                r = np.arange(i, min(i + g.shape[0], n))
                g[r - i, r] = np.inf
            cand = np.argsort(g, axis=1, kind="stable")[:, :min(n, 2 * 8)]              # ties: the lower index first
            # the Gram form picks, differences rank: (q - ref)^2 summed keeps its relative accuracy for a near copy
            e = ((q[i:i + rows, None, :] - ref[cand]) ** 2).sum(axis=2)
            e[np.take_along_axis(g, cand, axis=1) == np.inf] = np.inf
            order = np.lexsort((cand, e), axis=1)[:, :k]
            ci, ce = np.take_along_axis(cand, order, axis=1), np.take_along_axis(e, order, axis=1)
            kk = ci.shape[1]
            idx[i:i + rows, :kk] = np.where(ce < np.inf, ci, -1)
            d2[i:i + rows, :kk] = ce
    bad = ~np.isfinite(nq)
    idx[bad], d2[bad] = -1, np.nan
    return idx, d2


def nearest_chunk(q, ref, k, idx, d2, q_base=0, ref_base=0, exclude_self=False, merge=False):
    """One jck_knn_index_f32 call on contiguous fp32 device matrices: the k nearest rows of this `ref` chunk (global indices
    ref_base + j) into idx int64 [M,k] / d2 fp32 [M,k], merged with what they hold when `merge`."""
    from hipgan._lib import JckError, cur_stream, lib, load_library
    (m, d), n = q.shape, ref.shape[0]
    nbytes = load_library().jck_knn_index_ws_bytes(m, n)
    if nbytes == 0:
        raise JckError(f"nearest: {m} x {n} rows are outside what jck_knn_index_f32 takes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    lib.jck_knn_index_f32(q, m, ref, n, d, k, int(q_base), int(ref_base), int(bool(exclude_self)), int(bool(merge)), idx, d2, ws, cur_stream())


def segment_mean(x, labels, k, centre=None):
    """(sum fp32 [k,D], count int32 [k], centre fp32 [k,D]): per-cluster sums, sizes and means of the rows of x [N,D] under int64
    labels [N] (nearest's idx[:, 0:1] goes in as it is) - the update half of a Lloyd iteration.  Rows labelled outside 0..k-1 are
    skipped (nearest gives -1 to a non-finite row); an empty cluster has sum 0 and count 0 and keeps its row of `centre` (zeros
    where none was given); a non-empty one gets fp32 sum / fp32 count, correctly rounded.  centre is not modified: a new array leaves.
    CUDA (any argument a CUDA tensor): device tensors from jck_segment_mean_f32 (1 <= k <= 1024; no float atomics: the bits of
    sum[c] depend only on the rows labelled c, in ascending index); else numpy, the sums in fp64 and rounded to fp32 once - the
    same bits wherever the fp32 sums are exact."""
    k = int(k)
    if not 1 <= k <= 1024:
        raise ValueError(f"segment_mean: k = {k} needs 1 <= k <= 1024")
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"segment_mean: x must be a non-empty [rows, D] matrix, got {tuple(x.shape)}")
    n, d = x.shape
    if labels.ndim not in (1, 2) or labels.shape[0] != n or (labels.ndim == 2 and labels.shape[1] != 1):
        raise ValueError(f"segment_mean: labels must be [{n}] or [{n}, 1], got {tuple(labels.shape)}")
    if centre is not None and tuple(centre.shape) != (k, d):
        raise ValueError(f"segment_mean: centre must be [{k}, {d}], got {tuple(centre.shape)}")
    dev = _pair_device(x, labels, centre)
    if dev is not None:
        from hipgan._lib import JckError, cur_stream, lib, load_library
        x = _dev32(x, dev)
        lab = labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels, dtype=np.int64))
        lab = lab.detach().to(device=dev, dtype=torch.int64).contiguous()
        total = torch.empty(k, d, dtype=torch.float32, device=dev)
        count = torch.empty(k, dtype=torch.int32, device=dev)
        out = torch.zeros(k, d, dtype=torch.float32, device=dev) if centre is None else _dev32(centre, dev).clone()
        nbytes = load_library().jck_segment_ws_bytes(n, d, k)
        if nbytes == 0:
            raise JckError(f"segment_mean: {n} x {d} rows in {k} clusters are outside what jck_segment_mean_f32 takes")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        lib.jck_segment_mean_f32(x, n, d, lab, k, total, count, out, ws, cur_stream())
        return total, count, out
    x = _np64(x)
    lab = np.asarray(_host(labels), dtype=np.int64).reshape(-1)
    ok = (lab >= 0) & (lab < k)
    acc = np.zeros((k, d))
    np.add.at(acc, lab[ok], x[ok])
    total = acc.astype(np.float32)
    count = np.bincount(lab[ok], minlength=k).astype(np.int32)
    out = np.zeros((k, d), np.float32) if centre is None else np.array(_host(centre), dtype=np.float32)
    full = count > 0
    out[full] = total[full] / count[full].astype(np.float32)[:, None]
    return total, count, out


# ---- structural similarity of picture pairs (csrc/ssim.hip; the definition: DESIGN.md 5.16) -----------------------------------------
SSIM_C1, SSIM_C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _ssim_window():
    j = np.arange(11, dtype=np.float64)
    g = np.exp(-(j - 5.0) ** 2 / 4.5)
    return g / g.sum()


def _ssim_filter(p, g):
    """the separable 11-tap window over the valid region of the last two axes: [..., s, s] -> [..., s - 10, s - 10]"""
    m = p.shape[-1] - 10
    v = sum(g[j] * p[..., j:j + m, :] for j in range(11))
    return sum(g[j] * v[..., :, j:j + m] for j in range(11))


def _ssim_check(a, b, ia, ib, levels):
    from hipgan.diversity import default_levels, max_levels
    for name, x in (("a", a), ("b", b)):
        if x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2] or x.shape[0] < 1 or not 11 <= x.shape[1] <= 128:
            raise ValueError(f"ssim_pairs: {name} must be uint8 [n,S,S,3] with n >= 1 and 11 <= S <= 128, got {tuple(x.shape)}")
        if x.dtype not in (torch.uint8, np.uint8):
            raise ValueError(f"ssim_pairs: {name} must be uint8, got {x.dtype}")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"ssim_pairs: a is {a.shape[1]}x{a.shape[1]}, b is {b.shape[1]}x{b.shape[1]}")
    if ia.ndim != 1 or ib.ndim != 1 or ia.shape[0] != ib.shape[0] or not 1 <= ia.shape[0] <= 1 << 24:
        raise ValueError(f"ssim_pairs: ia and ib must be two index lists of one length 1..2^24, got {tuple(ia.shape)} and {tuple(ib.shape)}")
    S = int(a.shape[1])
    L = default_levels(S) if levels is None else int(levels)
    if not 1 <= L <= max_levels(S):
        raise ValueError(f"ssim_pairs: levels = {L} needs L >= 1, S % 2^(L-1) == 0 and S >> (L-1) >= 11 at S = {S}")
    return S, L


def ssim_pairs(a, b, ia, ib, levels=None, terms=False):
    """SSIM, multi-scale SSIM and squared error of the pairs (a[ia[p]], b[ib[p]]) of uint8 NHWC pictures [n,S,S,3], 11 <= S <= 128 (b may
    be a) -> {"ssim" [P], "ms_ssim" [P], "sq_err" int64 [P]} and, with terms, "terms" [P,3,L,2] = the means of the cs and ss maps per
    channel and level.  levels: L >= 1 with S % 2^(L-1) == 0 and S >> (L-1) >= 11; None: hipgan.diversity.default_levels(S).  A pair
    with an index outside its array gets NaN, NaN, -1.  CUDA (any argument a CUDA tensor): fp32 device tensors from jck_ssim_pairs_u8
    (one workgroup per pair, no float atomics; equal bits for swapped pictures, exactly 1, 1, 0 for equal ones); else numpy fp64."""
    as_np = lambda v: v if torch.is_tensor(v) else np.asarray(v)
    a, b, ia, ib = as_np(a), as_np(b), as_np(ia), as_np(ib)
    S, L = _ssim_check(a, b, ia, ib, levels)
    P = int(ia.shape[0])
    dev = _pair_device(a, b, ia, ib)
    if dev is not None:
        from hipgan._lib import cur_stream, lib
        u8 = lambda v: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).detach().to(dev).contiguous()
        ix = lambda v: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, dtype=np.int64))).detach().to(device=dev, dtype=torch.int64).contiguous()
        same = a is b
        a = u8(a)
        b = a if same else u8(b)
        out = {"ssim": torch.empty(P, dtype=torch.float32, device=dev), "ms_ssim": torch.empty(P, dtype=torch.float32, device=dev),
               "sq_err": torch.empty(P, dtype=torch.int64, device=dev)}
        if terms:
            out["terms"] = torch.empty(P, 3, L, 2, dtype=torch.float32, device=dev)
        lib.jck_ssim_pairs_u8(a, a.shape[0], b, b.shape[0], S, ix(ia), ix(ib), P, L, out["ssim"], out["ms_ssim"], out["sq_err"],
                              out.get("terms"), cur_stream())
        return out
    a, b = _host(a), _host(b)
    ia, ib = _host(ia).astype(np.int64), _host(ib).astype(np.int64)
    ok = (ia >= 0) & (ia < a.shape[0]) & (ib >= 0) & (ib < b.shape[0])
    g = _ssim_window()
    w = np.asarray(MS_SSIM_WEIGHTS[:L], dtype=np.float64)
    w = w / w.sum()
    t = np.full((P, 3, L, 2), np.nan)
    sq = np.full(P, -1, dtype=np.int64)
    rows = np.flatnonzero(ok)
    for lo in range(0, rows.shape[0], 64):                              # 64 pairs at a time: [64,3,S,S] fp64 planes
        r = rows[lo:lo + 64]
        xa, xb = a[ia[r]].astype(np.int64), b[ib[r]].astype(np.int64)
        sq[r] = ((xa - xb) ** 2).reshape(r.shape[0], -1).sum(axis=1)
        x, y = (np.moveaxis(v, 3, 1).astype(np.float64) for v in (xa, xb))
        for l in range(L):
            mx, my = _ssim_filter(x, g), _ssim_filter(y, g)
            vx, vy, vxy = _ssim_filter(x * x, g) - mx * mx, _ssim_filter(y * y, g) - my * my, _ssim_filter(x * y, g) - mx * my
            cs = (2.0 * vxy + SSIM_C2) / (vx + vy + SSIM_C2)
            ss = (2.0 * mx * my + SSIM_C1) / (mx * mx + my * my + SSIM_C1) * cs
            t[r, :, l, 0], t[r, :, l, 1] = cs.mean(axis=(2, 3)), ss.mean(axis=(2, 3))
            if l + 1 < L:
                x, y = (0.25 * (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2]) for v in (x, y))
    out = {"ssim": t[:, :, 0, 1].mean(axis=1), "ms_ssim": ms_ssim_from_terms(t), "sq_err": sq}
    if terms:
        out["terms"] = t
    return out


def ms_ssim_from_terms(t):
    """[P] from terms [P,3,L,2] (fp64 on the host): mean_c prod_{l<L-1} max(cs[c][l], 0)^w_l * max(ss[c][L-1], 0)^w_(L-1), w the first L
    of MS_SSIM_WEIGHTS over their sum"""
    t = _np64(t)
    L = t.shape[2]
    w = np.asarray(MS_SSIM_WEIGHTS[:L], dtype=np.float64)
    w = w / w.sum()
    with np.errstate(invalid="ignore"):
        f = np.concatenate([np.maximum(t[:, :, :L - 1, 0], 0.0), np.maximum(t[:, :, L - 1:, 1], 0.0)], axis=2) ** w
    return np.where(np.isnan(t).any(axis=(1, 2, 3)), np.nan, f.prod(axis=2).mean(axis=1))


def psnr(sq_err, S):
    """10 log10(255^2 * 3 S^2 / sq_err) in dB per pair, fp64 on the host: inf at 0, NaN for the -1 of a pair that was not compared"""
    e = _np64(sq_err)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10.0 * np.log10(255.0 ** 2 * 3 * int(S) ** 2 / e)
    return np.where(e < 0, np.nan, out)


# ---- sliced Wasserstein distance on Laplacian-pyramid patches (csrc/swd.hip; the definition: DESIGN.md 5.17) ------------------------
SWD_CHUNK = 4096        # pictures per launch of the device path: bounds the uint8 staging of host pictures (48 KB each at S = 128) and
#                         the fp64 partial rows of the statistics; the [L][D][n P] projection rows are whole whatever the chunk


def _swd_check(a, b, levels, patches, dirs, repeats):
    from hipgan.swd import SIZES, max_levels
    for name, x in (("a", a), ("b", b)):
        if x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2] or x.shape[0] < 1 or x.shape[1] not in SIZES:
            raise ValueError(f"swd: {name} must be uint8 [n,S,S,3] with n >= 1 and S in {SIZES}, got {tuple(x.shape)}")
        if x.dtype not in (torch.uint8, np.uint8):
            raise ValueError(f"swd: {name} must be uint8, got {x.dtype} {tuple(x.shape)}")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"swd: the two sets must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    S = int(a.shape[1])
    L = max_levels(S) if levels is None else int(levels)
    if not 1 <= L <= max_levels(S):
        raise ValueError(f"swd: levels = {L} must lie in 1..{max_levels(S)} at {tuple(a.shape)} (sides down to 16)")
    if int(patches) < 1 or int(dirs) < 1 or int(repeats) < 1:
        raise ValueError(f"swd: patches = {patches}, dirs = {dirs}, repeats = {repeats} must be >= 1 (pictures {tuple(a.shape)})")
    if int(a.shape[0]) * int(patches) >= 1 << 31:
        raise ValueError(f"swd: n * patches = {int(a.shape[0]) * int(patches)} keys a row must stay below 2^31 (pictures {tuple(a.shape)})")
    return S, L


def swd(a, b, levels=None, patches=128, dirs=128, repeats=4, seed=0, chunk=None):
    """Sliced Wasserstein distance between the Laplacian-pyramid patch statistics of two sets of uint8 NHWC pictures [n,S,S,3] of one
    shape, S in (32, 64, 128) -> {"swd" fp64 [L] (x 1e3, one number per level, finest first), "mean", "sides" [s_0 .. s_(L-1)],
    "per_repeat" fp64 [R][L]}.  levels: None = every level with side >= 16.  Per picture and level `patches` 7 x 7 x 3 patches, their
    corners and the `repeats` x `dirs` unit directions from hipgan.swd.draw(seed) - the same for both sets and for both paths.  CUDA (an
    argument a CUDA tensor): jck_swd_patch_stats_u8 / jck_swd_project_u8 / jck_sort_rows_f32 / jck_swd_rows, a repeat at a time with
    one [L][D][n P] fp32 projection buffer per set (sorted in place) and one sort workspace of that size, the pictures in chunks of
    `chunk` (None: SWD_CHUNK) whose rows go to the chunk's offset; else numpy fp64.  Equal sets give exactly 0, swapped sets equal
    bits, on both paths."""
    from hipgan import swd as H
    as_np = lambda v: v if torch.is_tensor(v) else np.asarray(v)
    a, b = as_np(a), as_np(b)
    S, L = _swd_check(a, b, levels, patches, dirs, repeats)
    n, P, D, R = int(a.shape[0]), int(patches), int(dirs), int(repeats)
    step = SWD_CHUNK if chunk is None else int(chunk)
    if step < 1:
        raise ValueError(f"swd: chunk = {step} must be >= 1")
    pos, directions = H.draw(n, S, L, P, D, R, seed)
    M = n * P
    dev = _pair_device(a, b)
    per_repeat = np.zeros((R, L))
    if dev is not None:
        from hipgan._lib import cur_stream, lib, load_library
        same = a is b
        piece = lambda x, lo: (x[lo:lo + step] if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x[lo:lo + step]))).detach().to(dev).contiguous()
        pos_t = torch.from_numpy(pos).to(dev)
        count = float(M * 49)
        norm = []
        for x in ((a,) if same else (a, b)):
            part = torch.empty(min(step, n), L, 3, 2, dtype=torch.float64, device=dev)
            tot, tot_sq = np.zeros((L, 3)), np.zeros((L, 3))
            for lo in range(0, n, step):                                           # the chunks' sums add on the host, in chunk order
                s1, s2 = torch.empty(L, 3, dtype=torch.float64, device=dev), torch.empty(L, 3, dtype=torch.float64, device=dev)
                xs = piece(x, lo)
                lib.jck_swd_patch_stats_u8(xs, xs.shape[0], S, L, pos_t[lo:lo + step], P, part, s1, s2, cur_stream())
                tot += s1.cpu().numpy()
                tot_sq += s2.cpu().numpy()
            mean, rstd = H.moments_from_sums(tot, tot_sq, count)
            norm.append((torch.from_numpy(mean.astype(np.float32)).to(dev), torch.from_numpy(rstd.astype(np.float32)).to(dev)))
        if same:
            norm.append(norm[0])
        rows = L * D
        ws_bytes = load_library().jck_sort_rows_ws_bytes(rows, M)
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
        bufs = [torch.empty(rows, M, dtype=torch.float32, device=dev) for _ in range(2)]
        w = torch.empty(rows, dtype=torch.float64, device=dev)
        for r in range(R):
            d_t = torch.from_numpy(directions[r]).to(dev)
            for x, (mean_t, rstd_t), buf in zip((a, b), norm, bufs):
                for lo in range(0, n, step):
                    xs = piece(x, lo)
                    lib.jck_swd_project_u8(xs, xs.shape[0], S, L, pos_t[lo:lo + step], P, d_t, D, mean_t, rstd_t, buf.data_ptr() + 4 * lo * P, M, cur_stream())
                lib.jck_sort_rows_f32(buf, rows, M, buf, ws, ws_bytes, cur_stream())
            lib.jck_swd_rows(bufs[0], bufs[1], rows, M, w, cur_stream())
            per_repeat[r] = 1e3 * w.cpu().numpy().reshape(L, D).mean(axis=1)
    else:
        a, b = _host(a), _host(b)
        la, lb = H.pyramid(a, L)[1], H.pyramid(b, L)[1]
        for l in range(L):
            xn = []
            for plane in (la[l], lb[l]):
                d = H.descriptors(plane, pos[:, l])
                mean, rstd = H.moments(d)
                xn.append(((d - mean[None, :, None]) * rstd[None, :, None]).reshape(M, H.DESC))
            for r in range(R):
                dr = directions[r].astype(np.float64).T
                sa, sb = np.sort(xn[0] @ dr, axis=0), np.sort(xn[1] @ dr, axis=0)
                per_repeat[r, l] = 1e3 * np.abs(sa - sb).mean(axis=0).mean()
    return H.report(per_repeat, S)


# ---- power spectra of pictures (csrc/spectrum.hip; the definition: DESIGN.md 5.18) -----------------------------------------------------
SPECTRUM_CHUNK = 4096   # pictures per launch of the device path: bounds the uint8 staging of host pictures; the derived bound of the mean
#                         plane counts on at most 2^12 pictures a launch


def spectrum(x, plane="luma", window=None, mean2d=False, chunk=None):
    """Power spectra of uint8 NHWC pictures [n,S,S,3], S in (32, 64, 128), n >= 0 -> {"profile" fp64 [n][R] (the azimuthally averaged
    power per radial bin, byte levels squared; R = 24 / 46 / 92), "mean" fp64 [n] (the plane's mean in byte levels), "radius" [R],
    "count" [R], "mean2d" fp64 [S][S] (the mean power plane; None unless asked for), "S", "plane", "window"}.  plane: "r", "g", "b",
    "luma" (or 0..3); window: None or "hann" (periodic; removes the leakage of the picture's borders).  A CUDA tensor runs
    jck_spectrum_u8, `chunk` pictures (None: SPECTRUM_CHUNK) a launch - profiles are bit-equal whatever the chunking, the chunks' plane
    sums add on the host in chunk order; anything else runs numpy fp64 (hipgan.spectrum.host_spectrum)."""
    from hipgan import spectrum as H
    x = x if torch.is_tensor(x) else np.asarray(x)
    if x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2] or x.shape[1] not in H.SIZES:
        raise ValueError(f"spectrum: x must be uint8 [n,S,S,3] with S in {H.SIZES}, got {tuple(x.shape)}")
    if x.dtype not in (torch.uint8, np.uint8):
        raise ValueError(f"spectrum: x must be uint8, got {x.dtype} {tuple(x.shape)}")
    pl, window = H.plane_index(plane), H.check_window(window)
    step = SPECTRUM_CHUNK if chunk is None else int(chunk)
    if step < 1:
        raise ValueError(f"spectrum: chunk = {step} must be >= 1")
    n, S = int(x.shape[0]), int(x.shape[1])
    dev = _pair_device(x)
    if dev is None:
        return H.host_spectrum(_host(x), pl, window, bool(mean2d), step)
    from hipgan._lib import cur_stream, lib, load_library
    R = H.bins(S)
    w, W = H.window_table(S, window)
    w_t = None if w is None else torch.from_numpy(w).to(dev)
    prof, mean = torch.empty(n, R, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    total = np.zeros((S, S))
    ws_bytes = load_library().jck_spectrum_ws_bytes(min(step, n), S, 1) if mean2d else 0
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=dev)
    plane_t = torch.empty(S, S, dtype=torch.float64, device=dev) if mean2d else None
    with torch.cuda.device(dev):
        for lo in range(0, n, step):
            xs = x[lo:lo + step].detach().contiguous()
            k = int(xs.shape[0])
            lib.jck_spectrum_u8(xs, k, S, pl, w_t, float(W), prof[lo:lo + k], mean[lo:lo + k], plane_t, ws if mean2d else None, ws_bytes, cur_stream())
            if mean2d:                                                             # one chunk: the kernel's plane as it is
                total = plane_t.cpu().numpy() if k == n else total + k * plane_t.cpu().numpy()
    return H.result(prof.cpu().numpy(), mean.cpu().numpy(), S, pl, window, (total if n <= step else total / n) if mean2d else None)


def spectrum_report(a, b):
    """two spectrum() dicts (a: samples, b: training pictures; their n may differ) -> the report of hipgan.spectrum.report: per radial bin
    mean_db / std_db of both sets, gap_db, z; rms_gap_db, high_gap_db, worst; with both mean planes the 15 lattice peaks and
    checkerboard_db; separability"""
    from hipgan.spectrum import report
    return report(a, b)


def _scalar(v):
    v = v.detach().cpu().numpy() if torch.is_tensor(v) else v
    return float(np.asarray(v, dtype=np.float64).reshape(-1)[0])


def _host(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def kid_from_sums(rr, ff, rf, m, n):
    """the unbiased MMD^2 from the three kernel sums (real x real and fake x fake without their diagonals) of m real and n fake rows"""
    return _scalar(rr) / (m * (m - 1)) + _scalar(ff) / (n * (n - 1)) - 2.0 * _scalar(rf) / (m * n)


def kid_from_features(real, fake):
    """Kernel Inception Distance of two feature matrices: sum_{i!=j} k(x_i,x_j) / (m(m-1)) + sum_{i!=j} k(y_i,y_j) / (n(n-1))
    - 2 sum k(x_i,y_j) / (mn) with k(a,b) = (a.b/D + 1)^3, over the full sets.  Non-finite features give NaN."""
    dev = _pair_device(real, fake)
    if dev is not None:
        real, fake = _dev32(real, dev), _dev32(fake, dev)
    small, big = (fake, real) if fake.shape[0] <= real.shape[0] else (real, fake)      # the kernel's grid runs over its second operand
    return kid_from_sums(poly3_sum(real, real, True), poly3_sum(fake, fake, True), poly3_sum(small, big), real.shape[0], fake.shape[0])


def precision_recall_from_hits(hit_fake, hit_real):
    """(precision, recall) from the hit vectors of fake in real's manifold and of real in fake's; a 255 marker (a non-finite row
    in either set) gives (nan, nan)"""
    hit_fake, hit_real = _host(hit_fake), _host(hit_real)
    if (hit_fake == 255).any() or (hit_real == 255).any():
        return float("nan"), float("nan")
    return float(hit_fake.mean()), float(hit_real.mean())


def precision_recall_from_features(real, fake, k=3):
    """Improved precision / recall: (mean hit of fake in real's k-NN manifold, mean hit of real in fake's).  A non-finite row in
    either set gives (nan, nan)."""
    dev = _pair_device(real, fake)
    if dev is not None:
        real, fake = _dev32(real, dev), _dev32(fake, dev)
    return precision_recall_from_hits(manifold_hit(fake, real, knn_radius2(real, k)), manifold_hit(real, fake, knn_radius2(fake, k)))


class Metrics:
    def __init__(self, real_images, extractor=None, real_features=None, cache="./data/metric_data.pikl"):
        self.device = get_default_device()
        self.class_to_superclass = {c: s for s, row in enumerate(SUPERCLASS_MEMBERS) for c in row}
        self.inception_model = extractor if extractor is not None else (None if real_features is not None
                                                                        else default_extractor(self.device))
        real_targets = getattr(real_images, "targets", None)
        fake_targets = [i for i in range(100) for _ in range(10)]
        self.real_superclass_idx, self.fake_superclass_idx = {}, {}
        for s in range(20):
            self.fake_superclass_idx[s] = [i for i, t in enumerate(fake_targets) if self.class_to_superclass[t] == s]
            if real_targets is not None:
                self.real_superclass_idx[s] = [i for i, t in enumerate(real_targets) if self.class_to_superclass[int(t)] == s]
        if real_features is not None:
            self.real_features = np.asarray(real_features)
        elif os.path.exists(cache):
            with open(cache, "rb") as f:
                self.real_features = pickle.load(f)
        else:
            loader = torch.utils.data.DataLoader(real_images, 128, shuffle=False, num_workers=0)
            self.real_features = self._extract(loader, real=True)
            os.makedirs(os.path.dirname(cache), exist_ok=True)
            with open(cache, "wb") as f:
                pickle.dump(self.real_features, f, pickle.HIGHEST_PROTOCOL)

    def _prep_real(self, image):
        """real images arrive as uint8 [B,3,32,32]: Resize((299,299)) + ImageNet normalisation (reference preprocessor :44-47)."""
        x = image.float() / 255.0 if image.dtype == torch.uint8 else image
        if x.shape[-1] != 299:
            x = torch.nn.functional.interpolate(x, size=[299, 299], mode="bilinear", align_corners=False)
            mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
            std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
            x = (x - mean) / std
        return x

    def _extract(self, images, real=False, softmax=False, keep_on_device=False):
        feats = []
        for image in images:
            if real:
                image = self._prep_real(image[0])
            if self.inception_model is None:
                feature = image if torch.is_tensor(image) else torch.as_tensor(image)     # pre-computed features
            else:
                with torch.no_grad():
                    feature = self.inception_model(image.to(self.device))
            if softmax:
                feature = torch.nn.functional.softmax(feature.float(), dim=1)
            feats.append(feature.detach())
        feats = torch.cat([f if torch.is_tensor(f) else torch.as_tensor(f) for f in feats])
        return feats if (keep_on_device and feats.is_cuda) else feats.cpu().numpy()

    # ---- one forward pass, every score (the evaluation branch of the trainers: the reference runs the network once per score on
    # the same images - metrics.py:98,114 - which yields the same features each time)
    def logits(self, images, batch=128):
        """images: a tensor [N,3,299,299] already prepared for the network (device or host) -> logits [N,100] where the
        extractor left them."""
        out = []
        for i in range(0, images.shape[0], batch):
            chunk = images[i:i + batch]
            if self.inception_model is None:
                out.append(chunk)
                continue
            with torch.no_grad():
                out.append(self.inception_model(chunk.to(self.device)).detach())
        return torch.cat(out)

    def fake_stats_device(self, logits, intra=False):
        """Device part of the FID of generated logits (CUDA): {'mu', 'cov'[, 'mu_s<k>', 'cov_s<k>' per superclass]} as fp64 device
        tensors - no host sync, so it can sit on a side stream; finish with scores_from_stats()."""
        out = {}
        out["mu"], out["cov"] = mean_cov_device(logits)
        if intra:
            for s_ in range(20):
                idx = torch.as_tensor(self.fake_superclass_idx[s_], device=logits.device)
                out[f"mu_s{s_}"], out[f"cov_s{s_}"] = mean_cov_device(logits[idx])
        return out

    def _real_stats(self, label=None):
        """(mean, cov) of the cached real features (of one superclass), computed once - on the device when there is one"""
        cache = self.__dict__.setdefault("_real_stats_cache", {})
        if label not in cache:
            dev = self._real_on_device()
            if label is None:
                cache[label] = mean_cov(dev if dev is not None else self.real_features)
            else:
                idx = self.real_superclass_idx[label]
                cache[label] = mean_cov(dev[torch.as_tensor(idx, device=dev.device)] if dev is not None else self.real_features[idx])
        return cache[label]

    def scores_from_stats(self, logits, stats, splits=10, intra=False):
        """Host part: logits (host) -> inception score; stats (host copies of fake_stats_device) -> FID[, intra-FID]."""
        probs = torch.nn.functional.softmax(torch.as_tensor(logits).float(), dim=1).numpy()
        is_ = inception_score_from_probs(probs, splits)
        g = lambda v: v.numpy() if torch.is_tensor(v) else v
        fid = fid_from_stats(*self._real_stats(), g(stats["mu"]), g(stats["cov"]))
        if not intra:
            return is_, fid
        total = sum(fid_from_stats(*self._real_stats(s_), g(stats[f"mu_s{s_}"]), g(stats[f"cov_s{s_}"])) for s_ in range(20))
        return is_, fid, total / 100

    def scores_from_logits(self, logits, splits=10, intra=False):
        """-> (inception score, FID[, intra-FID]) from the logits of the generated images; the same arithmetic as
        inception_score() / fid() / intra_fid()."""
        probs = torch.nn.functional.softmax(logits.float(), dim=1).cpu().numpy()
        is_ = inception_score_from_probs(probs, splits)
        on_dev = logits.is_cuda and self._real_on_device() is not None
        feats = logits if on_dev else logits.detach().cpu().numpy()
        fid = fid_from_features(self._real_on_device() if on_dev else self.real_features, feats)
        if not intra:
            return is_, fid
        total = 0
        for s_ in range(20):
            sub = feats[torch.as_tensor(self.fake_superclass_idx[s_], device=logits.device)] if on_dev else feats[self.fake_superclass_idx[s_]]
            idx = self.real_superclass_idx[s_]
            real = self._real_on_device()[torch.as_tensor(idx, device=logits.device)] if on_dev else self.real_features[idx]
            total += fid_from_features(real, sub)
        return is_, fid, total / 100

    def inception_score(self, images, splits=10):
        return inception_score_from_probs(self._extract(images, softmax=True), splits)

    def _real_on_device(self):
        """the cached real features, uploaded once when a GPU is there (their mean / covariance are then formed on it)"""
        if not torch.cuda.is_available():
            return None
        if getattr(self, "_real_dev", None) is None:
            self._real_dev = torch.as_tensor(np.asarray(self.real_features, dtype=np.float32)).to(self.device)
        return self._real_dev

    def fid(self, generated_images, intra_fid=False, label=0):
        gen = self._extract(generated_images, keep_on_device=True)
        dev = self._real_on_device() if (torch.is_tensor(gen) and gen.is_cuda) else None
        if intra_fid:
            idx = self.real_superclass_idx[label]
            real = dev[torch.as_tensor(idx, device=dev.device)] if dev is not None else self.real_features[idx]
        else:
            real = dev if dev is not None else self.real_features
        return fid_from_features(real, gen)

    def intra_fid(self, generated_images):
        total = 0
        for s in range(20):
            sub = generated_images[self.fake_superclass_idx[s]]
            total += self.fid(torch.utils.data.DataLoader(sub, 128, shuffle=False), intra_fid=True, label=s)
        return total / 100

    # ---- KID, intra-KID, precision / recall (not in the reference; the trainers report them with --extra_metrics 1)
    def _real_pair_stats(self, label=None, on_device=False):
        """Real-side terms of KID for all real features (label None) or one superclass, computed once per Metrics object:
        {'feats', 'n', 'rr' = sum_{i!=j} k(x_i, x_j)} - device tensors when on_device, else numpy / float."""
        cache = self.__dict__.setdefault("_real_pair_cache", {})
        key = (label, bool(on_device))
        if key not in cache:
            feats = self._real_on_device() if on_device else np.asarray(self.real_features, dtype=np.float32)
            if label is not None:
                idx = self.real_superclass_idx[label]
                feats = feats[torch.as_tensor(idx, device=feats.device)].contiguous() if on_device else feats[idx]
            cache[key] = {"feats": feats, "n": int(feats.shape[0]), "rr": poly3_sum(feats, feats, True)}
        return cache[key]

    def _real_radii(self, k=3, on_device=False):
        """squared k-NN radii of the real features (real's manifold), computed once per k"""
        cache = self.__dict__.setdefault("_real_radii_cache", {})
        key = (int(k), bool(on_device))
        if key not in cache:
            cache[key] = knn_radius2(self._real_pair_stats(None, on_device)["feats"], k)
        return cache[key]

    def fake_pair_stats_device(self, logits, intra=False, k=3):
        """Device part of KID / precision / recall of generated logits (CUDA), enqueued on the current stream without a host sync;
        finish with extra_scores_from_stats().  {'kid_rr', 'kid_ff', 'kid_rf'} fp64 sums [1], {'hit_fake', 'hit_real'} uint8 hit
        vectors (fake in real's manifold, real in fake's) and, with intra, 'kid_rr_s<k>', 'kid_ff_s<k>', 'kid_rf_s<k>' per superclass."""
        x = logits.detach().to(torch.float32).contiguous()
        real = self._real_pair_stats(None, True)
        out = {"kid_rr": real["rr"], "kid_ff": poly3_sum(x, x, True), "kid_rf": poly3_sum(x, real["feats"]),
               "hit_fake": manifold_hit(x, real["feats"], self._real_radii(k, True)),
               "hit_real": manifold_hit(real["feats"], x, knn_radius2(x, k))}
        if intra:
            for s_ in range(20):
                xs = x[torch.as_tensor(self.fake_superclass_idx[s_], device=x.device)].contiguous()
                rs = self._real_pair_stats(s_, True)
                out[f"kid_rr_s{s_}"], out[f"kid_ff_s{s_}"], out[f"kid_rf_s{s_}"] = rs["rr"], poly3_sum(xs, xs, True), poly3_sum(xs, rs["feats"])
        return out

    def extra_scores_from_stats(self, stats, intra=False):
        """Host part: host copies of fake_pair_stats_device -> {'kid', 'precision', 'recall'[, 'intra_kid']}."""
        m, n = int(np.asarray(self.real_features).shape[0]), int(stats["hit_fake"].shape[0])
        precision, recall = precision_recall_from_hits(stats["hit_fake"], stats["hit_real"])
        out = {"kid": kid_from_sums(stats["kid_rr"], stats["kid_ff"], stats["kid_rf"], m, n), "precision": precision, "recall": recall}
        if intra:
            out["intra_kid"] = float(np.mean([kid_from_sums(stats[f"kid_rr_s{s_}"], stats[f"kid_ff_s{s_}"], stats[f"kid_rf_s{s_}"],
                                                            len(self.real_superclass_idx[s_]), len(self.fake_superclass_idx[s_]))
                                              for s_ in range(20)]))
        return out

    def _kid_of(self, gen, label=None):
        on_dev = torch.is_tensor(gen) and gen.is_cuda and self._real_on_device() is not None
        real = self._real_pair_stats(label, on_dev)
        gen = _dev32(gen, real["feats"].device) if on_dev else _np64(gen)
        return kid_from_sums(real["rr"], poly3_sum(gen, gen, True), poly3_sum(gen, real["feats"]), real["n"], gen.shape[0])

    def kid(self, generated_images, intra_kid=False, label=0):
        """Kernel Inception Distance of the generated images against the cached real features (of superclass `label` with
        intra_kid), in the style of fid(); the real x real term is computed once and kept."""
        return self._kid_of(self._extract(generated_images, keep_on_device=True), label if intra_kid else None)

    def intra_kid(self, generated_images):
        """The MEAN of the 20 per-superclass KIDs.  Deliberately not the reference's intra-FID normalisation (20 values summed
        and divided by 100, metrics.py:141): a mean of 20 is what the name says, and KID has no reference value to stay
        comparable with."""
        return float(np.mean([self.kid(torch.utils.data.DataLoader(generated_images[self.fake_superclass_idx[s]], 128, shuffle=False),
                                       intra_kid=True, label=s) for s in range(20)]))

    def nearest_real(self, generated_images, k=3):
        """(idx int64 [n,k], d2 [n,k]): the k real images nearest to each generated image in the metric network's feature space,
        against the cached real features (metrics.nearest; on the device when the features are there)."""
        gen = self._extract(generated_images, keep_on_device=True)
        on_dev = torch.is_tensor(gen) and gen.is_cuda and self._real_on_device() is not None
        return nearest(gen, self._real_on_device() if on_dev else np.asarray(self.real_features), k)

    def precision_recall(self, generated_images, k=3):
        """(precision, recall) of the generated images against real's k-NN manifold and of the real features against theirs;
        real's radii are computed once per k and kept."""
        gen = self._extract(generated_images, keep_on_device=True)
        on_dev = torch.is_tensor(gen) and gen.is_cuda and self._real_on_device() is not None
        real = self._real_pair_stats(None, on_dev)["feats"]
        gen = _dev32(gen, real.device) if on_dev else _np64(gen)
        return precision_recall_from_hits(manifold_hit(gen, real, self._real_radii(k, on_dev)), manifold_hit(real, gen, knn_radius2(gen, k)))
