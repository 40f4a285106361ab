"""Nearest training images of samples, in pixel space: are these samples new, or copies of training pictures?

    r = nearest_images(samples_u8, train_u8, k=4)      # uint8 NHWC both; a 32x32 training set is upscaled as the trainers do
    r["idx"][i], r["rmse"][i]                          # the k nearest training images of sample i, their RMS pixel distance
    r["copy"][i]                                       # sample i is closer to a training image than any other training image is

Both sides become u8 / 127.5 - 1 fp32 rows on the device, the reference `chunk` images at a time (50 000 x 12 288 fp32 is 2.4 GB),
and go through jck_knn_index_f32 (csrc/knnindex.hip): candidates from the Gram form, distances recomputed from differences, so a
near copy's distance keeps its digits.  There is no tuned threshold: the `copy` flag compares a sample's nearest distance with the
leave-one-out nearest-neighbour distance of that training image inside the training set.
nearest_rows runs the same walk and flag on rows of another space - the discriminator's features (hipgan.probe,
Sampler.neighbours(space="d")), which also find a shifted, recoloured or mirrored training picture."""
import numpy as np
import torch

from ._lib import JckError


def load_reference_images(path):
    """The `images` array of an .npz as a reference set: uint8 [N,S,S,3], any S (checked against the samples later)."""
    with np.load(path) as f:
        if "images" not in f.files:
            raise JckError(f"{path}: no 'images' array (found {sorted(f.files)})")
        im = f["images"]
    if im.dtype != np.uint8 or im.ndim != 4 or im.shape[3] != 3 or im.shape[1] != im.shape[2] or im.shape[0] < 1:
        raise JckError(f"{path}: 'images' must be uint8 [N,S,S,3], got {im.dtype} {tuple(im.shape)}")
    return torch.from_numpy(im.copy())


def _check_u8(x, what):
    x = torch.as_tensor(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2] or x.shape[0] < 1:
        raise JckError(f"{what} must be uint8 NHWC [n,S,S,3], got {x.dtype} {tuple(x.shape)}")
    return x


def upscale_steps(ref_size, size, what="reference"):
    """how many exact 2x upscales (resize2x_pil_u8, the training transform) take a ref_size picture to size; JckError if none do"""
    steps, s = 0, int(ref_size)
    while s < size:
        s, steps = 2 * s, steps + 1
    if s != size:
        raise JckError(f"{what} images are {ref_size}x{ref_size}; the samples' {size}x{size} is not reachable by 2x upscales")
    return steps


def _rows(u8, steps, device):
    """uint8 NHWC [n,s,s,3] (host or device) -> fp32 [n, D] rows u8 / 127.5 - 1 on the device, upscaled `steps` times first"""
    if steps:
        from preprocess.dcgan_data_preprocessor import resize2x_pil_u8
        x = u8.cpu().permute(0, 3, 1, 2)
        for _ in range(steps):
            x = resize2x_pil_u8(x)
        u8 = x.permute(0, 2, 3, 1)
    return (u8.to(device).to(torch.float32) / 127.5 - 1.0).reshape(u8.shape[0], -1).contiguous()


def nearest_images(query_u8, ref_u8, k=4, chunk=8192, flag=True, device="cuda:0"):
    """query_u8 uint8 [n,S,S,3], ref_u8 uint8 [N,S,S,3] or a size that 2x upscales take to S (32x32 training data) ->
    {"idx": int64 [n,k], "d2": fp32 [n,k] squared distance in [-1, 1] units, "rmse": sqrt(d2 / D)} as host numpy arrays; with flag
    also "ref_nn_d2" fp32 [n] (the leave-one-out nearest-neighbour distance, inside the reference set, of the image idx[i,0]) and
    "copy" bool [n] = d2[i,0] < ref_nn_d2[i]."""
    from metrics import nearest_chunk
    if not torch.cuda.is_available():
        raise JckError("nearest_images needs a GPU: the HIP path has no CPU fallback")
    q8, r8 = _check_u8(query_u8, "query images"), _check_u8(ref_u8, "reference images")
    k, chunk = int(k), int(chunk)
    if not 1 <= k <= 8 or chunk < 1:
        raise JckError(f"nearest_images: 1 <= k <= 8 and chunk >= 1, got k = {k}, chunk = {chunk}")
    steps = upscale_steps(r8.shape[1], q8.shape[1])
    n, N = q8.shape[0], r8.shape[0]
    q = _rows(q8, 0, device)
    D = q.shape[1]

    def walk(rows, kk):
        idx = torch.empty(rows.shape[0], kk, dtype=torch.int64, device=device)
        d2 = torch.empty(rows.shape[0], kk, dtype=torch.float32, device=device)
        for lo in range(0, N, chunk):
            nearest_chunk(rows, _rows(r8[lo:lo + chunk], steps, device), kk, idx, d2, ref_base=lo, merge=lo > 0)
        return idx, d2

    idx, d2 = walk(q, k)
    out = {"idx": idx.cpu().numpy(), "d2": d2.cpu().numpy()}
    out["rmse"] = np.sqrt(out["d2"] / D)
    if flag:
        first = out["idx"][:, 0]
        rows = np.unique(first[first >= 0])
        nn = np.full(n, np.nan, np.float32)
        if rows.size:
            # the matched rows are not consecutive, so the index equality that exclude_self tests cannot name them: take their two
            # nearest rows instead and drop the row itself (a duplicate elsewhere stays, at distance 0)
            mi, md = walk(_rows(r8[torch.as_tensor(rows)], steps, device), 2)
            mi, md = mi.cpu().numpy(), md.cpu().numpy()
            loo = np.where(mi[:, 0] == rows, md[:, 1], md[:, 0])
            nn[first >= 0] = loo[np.searchsorted(rows, first[first >= 0])]
        out["ref_nn_d2"] = nn
        with np.errstate(invalid="ignore"):
            out["copy"] = out["d2"][:, 0] < nn
    return out


def nearest_rows(q, ref, k=4, chunk=8192, flag=True):
    """The walk of nearest_images on rows that already exist - fp32 device matrices q [n,D] and ref [N,D] of any feature space, the
    discriminator's for one (hipgan.probe.extract) -> {"idx", "d2"} and, with flag, "ref_nn_d2" and "copy" as nearest_images defines
    them; no "rmse": a feature distance has no pixel unit."""
    from metrics import nearest
    k, chunk = int(k), int(chunk)
    if not 1 <= k <= 8 or chunk < 1:
        raise JckError(f"nearest_rows: 1 <= k <= 8 and chunk >= 1, got k = {k}, chunk = {chunk}")
    n = q.shape[0]
    idx, d2 = nearest(q, ref, k, chunk=chunk)
    out = {"idx": idx.cpu().numpy(), "d2": d2.cpu().numpy()}
    if flag:
        first = out["idx"][:, 0]
        rows = np.unique(first[first >= 0])
        nn = np.full(n, np.nan, np.float32)
        if rows.size:
            # as in nearest_images: the matched rows' two nearest rows, the row itself dropped (a duplicate elsewhere stays, at 0)
            mi, md = nearest(ref[torch.as_tensor(rows, device=ref.device)], ref, 2, chunk=chunk)
            mi, md = mi.cpu().numpy(), md.cpu().numpy()
            loo = np.where(mi[:, 0] == rows, md[:, 1], md[:, 0])
            nn[first >= 0] = loo[np.searchsorted(rows, first[first >= 0])]
        out["ref_nn_d2"] = nn
        with np.errstate(invalid="ignore"):
            out["copy"] = out["d2"][:, 0] < nn
    return out


def neighbour_rows(query_u8, ref_u8, idx, steps=0):
    """[sample 0 | its k neighbours | sample 1 | ...] uint8 [n * (1 + k), S,S,3]: with grid_u8(..., per_row = 1 + k) one row per
    sample.  A missing neighbour (idx -1) is a black image."""
    q = np.asarray(query_u8)
    idx = np.asarray(idx)
    uniq, inv = np.unique(idx[idx >= 0], return_inverse=True)
    pics = _check_u8(ref_u8, "reference images")[torch.as_tensor(uniq, dtype=torch.int64)]
    if steps:
        from preprocess.dcgan_data_preprocessor import resize2x_pil_u8
        x = pics.permute(0, 3, 1, 2)
        for _ in range(steps):
            x = resize2x_pil_u8(x)
        pics = x.permute(0, 2, 3, 1)
    pics = pics.numpy()
    out = np.zeros((q.shape[0], 1 + idx.shape[1]) + q.shape[1:], np.uint8)
    out[:, 0] = q
    nb = np.zeros((idx.size,) + q.shape[1:], np.uint8)
    nb[np.flatnonzero(idx.reshape(-1) >= 0)] = pics[inv]
    out[:, 1:] = nb.reshape(idx.shape + q.shape[1:])
    return out.reshape((-1,) + q.shape[1:])
