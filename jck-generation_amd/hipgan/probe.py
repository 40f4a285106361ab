"""The discriminator as a feature extractor (Radford et al. 2016, section 5.1): what has D learned about the classes?

    layout, F = feature_layout(64, 4)                  # [(stage, col0, C, H)]: stage i's block is f[:, col0 : col0 + 16 * C]
    f = engine.features(images_u8)                     # fp32 [n, F] on the device (DcganEngine.features, csrc: jck_engine_features)
    r = knn_probe(engine, train_u8, train_labels, test_u8, test_labels, k=5)
    r["accuracy"], r["per_class"]                      # k-nearest-neighbour vote on block-normalised features

Every conv stage's activation is pooled to a grid x grid raster (jck_grid_pool), flattened cell-major, channel-minor - the NHWC order
of every activation here - and the stages' blocks are concatenated, stage 0 first.  The distance-based users (knn_probe,
Sampler.neighbours(space="d")) divide each block by its L2 norm first: without that the shallow block, pooled from the largest
raster, sets the distance."""
import numpy as np
import torch

from ._lib import JckError

POOL_MODES = {"max": 0, "mean": 1}                     # jck_grid_pool's mode
_BLOCK = 4096                                          # images per host-to-device piece of a feature extraction


def feature_layout(image_size, grid):
    """([(stage, col0, C, H)], F) of the feature rows of a discriminator for image_size (64 or 128) pooled to grid (1, 2 or 4): stage
    i has C = 64 * 2^i channels on an H x H raster (H = image_size / 2^(i+1), down to 4) and owns the grid^2 * C columns from col0;
    F is their sum, jck_engine_feature_dim's answer (960 grid^2 at 64 x 64, 1984 grid^2 at 128 x 128)."""
    if image_size not in (64, 128):
        raise JckError(f"feature_layout: image_size must be 64 or 128, got {image_size!r}")
    if grid not in (1, 2, 4):
        raise JckError(f"feature_layout: grid must be 1, 2 or 4, got {grid!r}")
    layout, col0, stage = [], 0, 0
    h = image_size // 2
    while h >= 4:
        c = 64 << stage
        layout.append((stage, col0, c, h))
        col0 += grid * grid * c
        h, stage = h // 2, stage + 1
    return layout, col0


def _block_width(layout, F):
    """grid^2 of a layout whose total is F"""
    c = sum(b[2] for b in layout)
    if c < 1 or F % c:
        raise JckError(f"features of {F} columns do not fit a layout of {c} channels")
    return F // c


def normalise_blocks(f, layout):
    """f [n, F] with every stage's block of every row divided by that block's L2 norm (a torch op on f's device; a new tensor).  A
    zero block stays zero, a non-finite block stays non-finite."""
    f = torch.as_tensor(f)
    if f.dim() != 2:
        raise JckError(f"normalise_blocks: features must be [n, F], got {tuple(f.shape)}")
    g2 = _block_width(layout, f.shape[1])
    out = torch.empty_like(f)
    for _, col0, c, _ in layout:
        b = f[:, col0:col0 + g2 * c]
        nrm = torch.linalg.vector_norm(b, dim=1, keepdim=True)
        out[:, col0:col0 + g2 * c] = b / torch.where(nrm == 0, torch.ones_like(nrm), nrm)
    return out


def knn_vote(idx, labels, n_class):
    """int64 [n]: the majority class among each row's neighbours idx[i, :] >= 0 (nearest first) of the reference labels; a tie goes
    to the tied class whose first member is nearest; a row without neighbours gives -1.  numpy."""
    idx, labels = np.asarray(idx), np.asarray(labels).astype(np.int64).reshape(-1)
    if idx.ndim != 2:
        raise JckError(f"knn_vote: idx must be [n, k], got {idx.shape}")
    if labels.size and (labels.min() < 0 or labels.max() >= n_class):
        raise JckError(f"knn_vote: labels must lie in [0, {n_class})")
    n, k = idx.shape
    ok = idx >= 0
    cls = np.where(ok, labels[np.where(ok, idx, 0)], 0)
    votes = np.zeros((n, n_class), np.int64)
    np.add.at(votes, (np.repeat(np.arange(n), k)[ok.reshape(-1)], cls.reshape(-1)[ok.reshape(-1)]), 1)
    best = votes.max(axis=1, keepdims=True)
    pred = np.full(n, -1, np.int64)
    # the first neighbour, nearest first, whose class holds the most votes
    winner = ok & (np.take_along_axis(votes, cls, axis=1) == best)
    has = winner.any(axis=1)
    pred[has] = cls[has, winner[has].argmax(axis=1)]
    return pred


def _to_size(u8, size, what):
    """uint8 NHWC images of `size`, or of a size that exact 2x upscales (the training transform) take there"""
    from .neighbours import _check_u8, upscale_steps
    x = _check_u8(u8, what)
    steps = upscale_steps(x.shape[1], size, what)
    if steps:
        from preprocess.dcgan_data_preprocessor import resize2x_pil_u8
        x = x.cpu().permute(0, 3, 1, 2)
        for _ in range(steps):
            x = resize2x_pil_u8(x)
        x = x.permute(0, 2, 3, 1)
    return x


def extract(engine, images_u8, grid=4, pool="max", normalise="block"):
    """fp32 [n, F] on the engine's device: engine.features of uint8 NHWC images (the discriminator's size, or 32 x 32 data upscaled as
    the trainers do), a piece at a time so that only the features of a large set stay on the device; block-normalised unless
    normalise="none"."""
    if normalise not in ("block", "none"):
        raise JckError(f"normalise must be 'block' or 'none', got {normalise!r}")
    from .neighbours import _check_u8
    x = _check_u8(images_u8, "images")
    layout, F = feature_layout(engine.size, grid)
    out = torch.empty(x.shape[0], F, dtype=torch.float32, device=engine.device)
    for lo in range(0, x.shape[0], _BLOCK):
        f = engine.features(_to_size(x[lo:lo + _BLOCK], engine.size, "images"), grid=grid, pool=pool)
        out[lo:lo + _BLOCK] = f if normalise == "none" else normalise_blocks(f, layout)
    return out


def load_images(path, need_labels=False):
    """(uint8 tensor [n,S,S,3], int64 class ids [n] or None) of an .npz with an `images` array of any S and, required with need_labels,
    a `labels` array of class ids"""
    from .neighbours import load_reference_images
    u8 = load_reference_images(path)
    with np.load(path) as f:
        labels = f["labels"] if "labels" in f.files else None
    if labels is None and need_labels:
        raise JckError(f"{path}: no 'labels' array: the probe needs the class id of every picture")
    if labels is not None:
        labels = np.asarray(labels).reshape(-1).astype(np.int64)
        if labels.shape[0] != u8.shape[0]:
            raise JckError(f"{path}: {labels.shape[0]} labels for {u8.shape[0]} images")
    return u8, labels


def _class_ids(labels, n, what):
    lab = np.asarray(torch.as_tensor(labels).cpu()).reshape(-1).astype(np.int64)
    if lab.shape[0] != n:
        raise JckError(f"knn_probe: {lab.shape[0]} {what} labels for {n} images")
    if lab.min() < 0:
        raise JckError(f"knn_probe: {what} labels must be class ids >= 0")
    return lab


def knn_probe(engine, train_u8, train_labels, test_u8, test_labels, k=5, grid=4, pool="max", chunk=8192, normalise="block"):
    """A k-nearest-neighbour classifier on the discriminator's features: every test image takes the majority class (knn_vote) of its k
    nearest training images in feature space (metrics.nearest, the training features on the device, walked `chunk` rows at a time).
    -> {"accuracy": float, "pred": int64 [m], "idx": int64 [m,k], "d2": fp32 [m,k], "per_class": {class id: accuracy}} (host)."""
    from metrics import nearest
    k = int(k)
    if not 1 <= k <= 8:
        raise JckError(f"knn_probe: k = {k} needs 1 <= k <= 8")
    if int(chunk) < 1:
        raise JckError(f"knn_probe: chunk = {chunk} must be >= 1")
    n, m = torch.as_tensor(train_u8).shape[0], torch.as_tensor(test_u8).shape[0]
    ltr, lte = _class_ids(train_labels, n, "training"), _class_ids(test_labels, m, "test")
    train_f = extract(engine, train_u8, grid, pool, normalise)
    test_f = extract(engine, test_u8, grid, pool, normalise)
    idx, d2 = nearest(test_f, train_f, k, chunk=int(chunk))
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    pred = knn_vote(idx, ltr, int(max(ltr.max(), lte.max())) + 1)
    hit = pred == lte
    per_class = {int(c): float(hit[lte == c].mean()) for c in np.unique(lte)}
    return {"accuracy": float(hit.mean()), "pred": pred, "idx": idx, "d2": d2, "per_class": per_class}
