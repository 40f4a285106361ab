"""Input pipeline with the reference's interface (preprocess/dcgan_data_preprocessor.py): `DCGANDataPreprocessor(args)`,
`transform_data()`, `get_data_loader() -> (train_loader, metric_source)`.

The reference downloads CIFAR-100 through torchvision (no network / no torchvision here).  This version reads a LOCAL
copy of the CIFAR-100 python pickle (`./data/cifar-100-python/train`, the very file torchvision unpacks) when present and
otherwise falls back to seeded synthetic images of the same shape and range - the training hot path is identical.

MI355X-first layout: the uint8 dataset (150 MB for CIFAR) is copied to HBM ONCE; a batch is a vector of indices
(`hipgan.engine.DeviceBatch`) and the step itself gathers it and applies Resize(64) / ToTensor / Normalize(0.5, 0.5)
(reference :38-43) in the kernel that also adds the instance noise - no per-step host->device image traffic, no DataLoader
workers.  The transform is bit-exact against the reference's: transforms.Resize on a PIL image is PIL's bilinear resize,
whose 2x upscale is a horizontal and a vertical 3:1 pass each rounded to uint8 (`resize2x_pil_u8`, pinned to PIL by
tests/golden/resize_u8.json).  Without a GPU (and with JCKGAN_DEVICE_DATA=0) the same arithmetic runs as tensor ops on the
host and a torch DataLoader is returned, as in the reference.

Opt-in (main.py --data / --image_size / --mirror): any uint8 image set from an `images.npz` (`load_npz_dataset`) instead of CIFAR-100,
resized to 64x64 or 128x128 from any source size with Pillow's general bilinear taps (`resize_pil_u8` on the host,
jck_img_prep_u8_any in the step; pinned to PIL by tests/golden/resize_any_u8.json), and left-right flips drawn per epoch
(`DeviceLoader(mirror=True)`, device-resident pipeline only).  --crop center|random [--crop_size K] puts CenterCrop(K) / RandomCrop(K) in
front of the Resize: a K x K box of every image (`center_origin`; random origins drawn per epoch by `DeviceLoader(crop="random")`,
device-resident pipeline only) is what jck_img_prep_u8_box resizes, pinned to PIL's crop().resize() by tests/golden/crop_resize_u8.json;
evaluation reads the centre box of the same size."""
import math
import os
import pickle

import numpy as np
import torch

from logger.main_logger import MainLogger

CIFAR_DIR = os.path.join(".", "data", "cifar-100-python")
RESIZE_MAX_SRC = 1024              # include/jckgan.h: JCK_RESIZE_MAX_SRC


class _TensorSource:
    """metric source: tensor dataset with `.targets` (what metrics.Metrics reads, reference metrics.py:56)."""

    def __init__(self, images, targets):
        self.images, self.targets = images, targets

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        return self.images[i], self.targets[i]


def resize2x_pil_u8(x):
    """uint8 [..., H, W] -> uint8 [..., 2H, 2W] exactly as PIL.Image.resize(BILINEAR) upsamples by 2 (what
    transforms.Resize(64) does to a 32x32 PIL image, reference :39): horizontal pass, then vertical pass, each rounded to
    uint8; interior taps weigh 3:1, the clamped border taps reduce to a copy."""
    def up(t, dim):
        t = t.to(torch.int32).movedim(dim, -1)
        n = t.shape[-1]
        prev = torch.cat([t[..., :1], t[..., :-1]], -1)
        nxt = torch.cat([t[..., 1:], t[..., -1:]], -1)
        out = torch.empty(t.shape[:-1] + (2 * n,), dtype=torch.int32)
        out[..., 0::2] = (prev + 3 * t + 2) >> 2
        out[..., 1::2] = (3 * t + nxt + 2) >> 2
        return out.movedim(-1, dim)
    return up(up(x, -1), -2).to(torch.uint8)


def _axis_taps(length, size):
    """Pillow's bilinear taps of one axis (ImagingResample: precompute_coeffs + normalize_coeffs_8bpc) -> (lo [size], k [size, K]
    int64 weights in units of 2^-22, zero past an output's last tap).  Python floats are IEEE doubles and every operation below is
    rounded on its own, as in Pillow's C: the same integers (jck_resize_taps_build computes them for the device kernel)."""
    scale = length / size
    support = max(scale, 1.0)
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / support
    lo = torch.zeros(size, dtype=torch.int64)
    k = torch.zeros(size, ksize, dtype=torch.int64)
    for o in range(size):
        center = (o + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), length) - first
        w = [max(1.0 - abs((j + first - center + 0.5) * ss), 0.0) for j in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        lo[o] = first
        for j, v in enumerate(w):
            k[o, j] = int(0.5 + (v / ww if ww != 0.0 else v) * (1 << 22))
    return lo, k


def resize_pil_u8(x, size):
    """uint8 [..., H, W] -> uint8 [..., size, size] exactly as PIL.Image.resize((size, size), BILINEAR) (what transforms.Resize does
    to a PIL image): a horizontal pass, then a vertical pass on its result, each a fixed-point weighted sum rounded to uint8:
    out[o] = clip((2^21 + sum_j k[o][j] * src[lo[o] + j]) >> 22, 0, 255).  Any H, W >= 1; an axis that already has `size` entries is
    reproduced.  The host statement of the device kernel img_prep_u8_any_kernel; at 2x it is resize2x_pil_u8."""
    def one_axis(t, dim):
        t = t.to(torch.int64).movedim(dim, -1)
        length = t.shape[-1]
        lo, k = _axis_taps(length, size)
        acc = torch.full(t.shape[:-1] + (size,), 1 << 21, dtype=torch.int64)
        for j in range(k.shape[1]):
            acc += k[:, j] * t[..., (lo + j).clamp_(max=length - 1)]          # (a tap past the last one has weight 0)
        return (acc >> 22).clamp_(0, 255).movedim(-1, dim)
    return one_axis(one_axis(x, -1), -2).to(torch.uint8)


def center_origin(hs, ws, hc, wc):
    """Top-left corner (y0, x0) of the centred hc x wc box of an hs x ws image, as torchvision's center_crop places it:
    int(round(difference / 2.0)) with Python's round-half-to-even (12 for a difference of 25, 4 for 7)."""
    return int(round((hs - hc) / 2.0)), int(round((ws - wc) / 2.0))


def crop_side(crop, crop_size, hs, ws):
    """The side K of the square box of --crop / --crop_size for hs x ws images: None without a crop, min(hs, ws) - the largest
    centred square - when no size is given.  ValueError for a mode that does not exist, a size without a mode and a K outside
    1..min(hs, ws)."""
    if crop is None:
        if crop_size is not None:
            raise ValueError("crop_size needs a crop mode: crop must be 'center' or 'random'")
        return None
    if crop not in ("center", "random"):
        raise ValueError(f"crop must be 'center' or 'random', got {crop!r}")
    k = min(hs, ws) if crop_size is None else int(crop_size)
    if not 1 <= k <= min(hs, ws):
        raise ValueError(f"crop_size {k}: a square crop of {hs}x{ws} images has a side of 1..{min(hs, ws)}")
    return k


class DeviceLoader:
    """Iterable with the DataLoader surface the trainers use (`len()`, iteration over `[images, (labels)]` batches): images
    are `DeviceBatch`es over the uint8 dataset in HBM, labels (CGAN: int64 one-hot [B,100]) are gathered on the device.
    Shuffles every epoch like DataLoader(shuffle=True); under torch.distributed every rank takes a strided share of the same
    permutation (DistributedSampler semantics, padded by wrap-around).
    size: the side the step resizes to (64 or 128).  mirror: every drawn index also draws a left-right flip with probability 1/2
    (RandomHorizontalFlip) from a SECOND generator, so the index order of a seed is the same with and without it.
    crop: None, "center" or "random", crop_size: the side K of the square box (None: min(H, W)).  "center" resizes the centred
    K x K box of every image; "random" draws one origin per drawn index, y0 uniform on 0..H-K and x0 on 0..W-K, anew each epoch
    from a THIRD generator, so indices and flips of a seed do not depend on it either."""

    def __init__(self, data_u8, batch_size, onehot=None, seed=0, size=64, mirror=False, crop=None, crop_size=None):
        from hipgan.engine import DeviceBatch
        self._DeviceBatch = DeviceBatch
        self.data, self.onehot, self.batch_size = data_u8, onehot, batch_size
        self.size, self.mirror = size, bool(mirror)
        self.rank, self.world = 0, 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.rank, self.world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        self.n_local = (data_u8.shape[0] + self.world - 1) // self.world
        self.gen = torch.Generator().manual_seed(seed)
        self.flip_gen = torch.Generator().manual_seed(seed + 0x6d6972) if self.mirror else None
        self.crop = crop
        self.crop_size = crop_side(crop, crop_size, int(data_u8.shape[2]), int(data_u8.shape[3]))
        self.origin_gen = torch.Generator().manual_seed(seed + 0x63726f70) if crop == "random" else None

    def __len__(self):
        return (self.n_local + self.batch_size - 1) // self.batch_size

    def draw_epoch(self):
        """One epoch's draws of this rank on the host: (indices int64 [n_local], flips uint8 [n_local] or None, box origins int32
        [n_local,2] = (y0, x0) or None).  Every draw belongs to its position in the permutation, so all three are strided and
        wrapped alike."""
        n, (h, w), k = self.data.shape[0], self.data.shape[2:], self.crop_size
        perm = torch.randperm(n, generator=self.gen)
        flips = torch.randint(0, 2, (n,), generator=self.flip_gen, dtype=torch.uint8) if self.mirror else None      # one per drawn index, new every epoch
        origins = None
        if self.origin_gen is not None:
            origins = torch.stack([torch.randint(0, h - k + 1, (n,), generator=self.origin_gen, dtype=torch.int32),
                                   torch.randint(0, w - k + 1, (n,), generator=self.origin_gen, dtype=torch.int32)], 1)
        if self.world > 1:
            total = self.n_local * self.world
            perm, flips, origins = (torch.cat([t, t[:total - n]])[self.rank:total:self.world] if t is not None else None
                                    for t in (perm, flips, origins))
        return perm, flips, origins

    def __iter__(self):
        perm, flips, origins = (t.to(self.data.device) if t is not None else None for t in self.draw_epoch())
        k = self.crop_size
        center = (k, k, center_origin(*self.data.shape[2:], k, k)) if self.crop == "center" else None
        for i in range(0, perm.numel(), self.batch_size):
            idx = perm[i:i + self.batch_size]
            box = (k, k, origins[i:i + self.batch_size].contiguous()) if origins is not None else center
            batch = [self._DeviceBatch(self.data, idx, self.size, flips[i:i + self.batch_size] if flips is not None else None, box)]
            if self.onehot is not None:
                batch.append(self.onehot[idx])
            yield batch


def load_npz_dataset(path, need_labels=False):
    """--data FILE.npz, the format generate.py writes: `images` uint8 [N,H,W,3] (1 <= H, W <= 1024) and optionally `labels` int [N]
    -> (uint8 [N,3,H,W] planar host tensor, list of int labels or None).  need_labels (CGAN): `labels` must be there, all within
    0..99.  Everything is checked here, on the host, before anything is allocated on the device."""
    with np.load(path, allow_pickle=False) as z:
        if "images" not in z.files:
            raise ValueError(f"{path}: no `images` array (expected uint8 [N,H,W,3], as generate.py writes it)")
        img = z["images"]
        lab = z["labels"] if "labels" in z.files else None
    if img.dtype != np.uint8 or img.ndim != 4 or img.shape[3] != 3 or img.shape[0] < 1:
        raise ValueError(f"{path}: `images` must be uint8 [N,H,W,3] with N >= 1, got {img.dtype} {img.shape}")
    if not (1 <= img.shape[1] <= RESIZE_MAX_SRC and 1 <= img.shape[2] <= RESIZE_MAX_SRC):
        raise ValueError(f"{path}: images of {img.shape[1]}x{img.shape[2]}: the input pipeline takes 1..{RESIZE_MAX_SRC} pixels a side")
    if lab is None:
        if need_labels:
            raise ValueError(f"{path}: no `labels` array: the conditional model needs one class in 0..99 per image")
        labels = None
    else:
        if lab.ndim != 1 or lab.shape[0] != img.shape[0] or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError(f"{path}: `labels` must be int [{img.shape[0]}], got {lab.dtype} {lab.shape}")
        if need_labels and (int(lab.min()) < 0 or int(lab.max()) > 99):
            raise ValueError(f"{path}: `labels` must lie in 0..99, got {int(lab.min())}..{int(lab.max())}")
        labels = [int(t) for t in lab]
    return torch.from_numpy(np.ascontiguousarray(img.transpose(0, 3, 1, 2))), labels


class DCGANDataPreprocessor:
    NEED_LABELS = False

    def __init__(self, args, synthetic_size=None):
        self._logger = MainLogger(args)
        self.batch_size = args.batch_size
        self.num_worker = args.num_worker
        # the opt-in flags of main.py (absent from the namespace unless given): another dataset, the 128x128 topology, flips
        self.data_file = getattr(args, "data", None)
        self.image_size = int(getattr(args, "image_size", 64))
        self.mirror = bool(int(getattr(args, "mirror", 0)))
        if self.image_size not in (64, 128):
            raise ValueError(f"image_size must be 64 or 128, got {self.image_size}")
        self.crop, crop_size = getattr(args, "crop", None), getattr(args, "crop_size", None)
        self.metric_cache = None
        self.images, self.targets = self._load(synthetic_size)
        # the square box of --crop (None without one): checked here, on the host, before anything is allocated on the device
        self.crop_size = crop_side(self.crop, crop_size, int(self.images.shape[2]), int(self.images.shape[3]))
        if self.crop is not None:                   # features of the real images are those of ONE box: never another crop's cache
            base = self.metric_cache or os.path.join(".", "data", "metric_data.pikl")
            self.metric_cache = f"{os.path.splitext(base)[0]}_crop{self.crop_size}.pikl"
        self._train, self._metric = None, None
        self._logger.debug("data preprocessor init")

    def _load(self, synthetic_size):
        if self.data_file is not None:
            x, labels = load_npz_dataset(self.data_file, self.NEED_LABELS)
            # the real-feature cache of metrics.Metrics belongs to ONE dataset: ./data/metric_data.pikl holds CIFAR-100's
            st = os.stat(self.data_file)
            stem = os.path.splitext(os.path.basename(self.data_file))[0]
            self.metric_cache = os.path.join(".", "data", f"metric_{stem}_{st.st_size}_{st.st_mtime_ns}.pikl")
            self._logger.debug(f"dataset loaded from {self.data_file}: {tuple(x.shape)}" + ("" if labels is not None else ", no labels"))
            return x, labels if labels is not None else [0] * x.shape[0]
        path = os.path.join(CIFAR_DIR, "train")
        if synthetic_size is None and os.path.exists(path):
            with open(path, "rb") as f:
                d = pickle.load(f, encoding="latin1")
            x = torch.from_numpy(np.asarray(d["data"], dtype=np.uint8).reshape(-1, 3, 32, 32))
            self._logger.debug(f"CIFAR-100 loaded from {path}: {tuple(x.shape)}")
            return x, [int(t) for t in d["fine_labels"]]
        if synthetic_size is None and os.environ.get("JCKGAN_SYNTHETIC", "0") != "1":
            # a training run on random pixels must be asked for: silently writing checkpoints of a model trained on noise
            # because a path was mistyped helps nobody (the reference downloads CIFAR-100; there is no network here)
            raise FileNotFoundError(f"no local CIFAR-100 under {CIFAR_DIR} (expected the pickle `train` of cifar-100-python); "
                                    f"set JCKGAN_SYNTHETIC=1 to train on seeded synthetic 32x32 images instead")
        n = synthetic_size or 50000
        g = torch.Generator().manual_seed(2024)
        self._logger.warning(f"no local CIFAR-100 under {CIFAR_DIR}: using {n} seeded synthetic 32x32 images")
        x = (torch.rand(n, 3, 32, 32, generator=g) * 255).to(torch.uint8)
        return x, torch.randint(0, 100, (n,), generator=g).tolist()

    @staticmethod
    def device_resident():
        return torch.cuda.is_available() and os.environ.get("JCKGAN_DEVICE_DATA", "1") != "0"

    def transform_data(self):
        center = self.images
        if self.crop is not None:                                                 # CenterCrop(K); evaluation reads it in both modes
            k = self.crop_size
            y0, x0 = center_origin(*self.images.shape[2:], k, k)
            center = self.images[:, :, y0:y0 + k, x0:x0 + k].contiguous()
        self._metric = _TensorSource(center, self.targets)                        # 299x299 resize is done lazily by metrics.py
        if self.device_resident():
            self._train = self.images.cuda().contiguous()                         # uint8, transformed inside the step
        else:
            if self.mirror:
                raise ValueError("--mirror 1 needs the device-resident pipeline (a GPU, JCKGAN_DEVICE_DATA not 0): the host "
                                 "loader transforms the dataset once, before training, and has no per-step flip")
            if self.crop == "random":
                raise ValueError("--crop random needs the device-resident pipeline (a GPU, JCKGAN_DEVICE_DATA not 0): the host "
                                 "loader transforms the dataset once, before training, and cannot draw a crop per epoch")
            if tuple(center.shape[2:]) == (32, 32) and self.image_size == 64:
                up = resize2x_pil_u8(center)                                      # Resize(64) on the PIL image (:39)
            else:
                up = resize_pil_u8(center, self.image_size)                       # Resize((S, S)) of any source size, or of its centre box
            self._train = (up.float() / 255.0 - 0.5) / 0.5                        # ToTensor, Normalize(0.5, 0.5)
        self._logger.debug("data transform")

    def _device_loader(self, onehot=None):
        return DeviceLoader(self._train, self.batch_size, onehot=onehot, seed=12345, size=self.image_size, mirror=self.mirror,
                            crop=self.crop, crop_size=self.crop_size)

    def get_data_loader(self):
        if self._train is None:
            self.transform_data()
        if self._train.dtype == torch.uint8:
            return self._device_loader(), self._metric
        ds = torch.utils.data.TensorDataset(self._train)
        sampler = None
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            sampler = torch.utils.data.distributed.DistributedSampler(ds, shuffle=True)
        loader = torch.utils.data.DataLoader(ds, self.batch_size, shuffle=sampler is None, sampler=sampler,
                                             num_workers=self.num_worker, pin_memory=torch.cuda.is_available())
        return loader, self._metric
