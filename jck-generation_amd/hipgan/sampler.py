"""Generator inference outside the trainer: load a checkpoint's generator into a step engine of its own and draw images.

    s = Sampler.from_checkpoint("best.pt", "DCGAN")          # the averaged generator when the file has one
    u8 = s.images(1000, seed=0, truncation=0.7)                # uint8 [1000,S,S,3] on the device

Sampling runs with bn="running" by default (DcganEngine.sample): BatchNorm on the running statistics, every image a function of
its own z, any n.  The running statistics of an AVERAGED generator were never fitted to its weights - they are the live ones at
the moment the average was seeded plus a handful of momentum-0.1 updates from evaluation sampling - so call calibrate() first
when sampling `which="ema"` that way.  The latent helpers (truncated z, slerp) are host code: z is tiny."""
import math

import torch

from ._lib import JckError

N_CLASS, NZ = 100, 100


def pick_generator_state(ckpt, which="auto"):
    """The generator state dict of a checkpoint dict (the trainer's or the reference's: 'model_g', and 'model_g_ema' where the
    run kept an average) -> (state dict, "live" | "ema")."""
    if not isinstance(ckpt, dict) or "model_g" not in ckpt:
        raise JckError("checkpoint has no 'model_g' entry: not a trainer checkpoint")
    if which not in ("auto", "live", "ema"):
        raise JckError(f"which must be 'auto', 'live' or 'ema', got {which!r}")
    if which == "ema" and "model_g_ema" not in ckpt:
        raise JckError("checkpoint has no 'model_g_ema': the run kept no averaged generator (--ema_decay)")
    if which == "ema" or (which == "auto" and "model_g_ema" in ckpt):
        return ckpt["model_g_ema"], "ema"
    return ckpt["model_g"], "live"


def image_size_of(g_state):
    """64 for the reference's five-layer generator, 128 for the six-layer plan."""
    n = sum(1 for k in g_state if k.startswith("conv") and k.endswith(".weight"))
    if n not in (5, 6):
        raise JckError(f"generator state has {n} conv layers; 5 (64x64) or 6 (128x128) expected")
    return 64 if n == 5 else 128


def latents(n, seed, truncation=None):
    """z [n,100] fp32 on the host from a seeded torch.Generator; truncation t: a standard normal truncated to [-t, t]
    (torch.nn.init.trunc_normal_)."""
    g = torch.Generator().manual_seed(int(seed))
    if truncation is None:
        return torch.randn(n, NZ, generator=g)
    t = float(truncation)
    if not t > 0.0:
        raise JckError(f"truncation must be > 0, got {truncation}")
    return torch.nn.init.trunc_normal_(torch.empty(n, NZ), mean=0.0, std=1.0, a=-t, b=t, generator=g)


def slerp(z0, z1, steps):
    """Spherical interpolation z0 -> z1 in `steps` points, both ends included: [steps, ...] (rows of norm |z0| = |z1| keep it).
    Falls back to the straight line when the two are (anti)parallel."""
    if steps < 2:
        raise JckError("interpolate: steps >= 2")
    a, b = z0.detach().double().reshape(-1), z1.detach().double().reshape(-1)
    if a.shape != b.shape:
        raise JckError("interpolate: z0 and z1 differ in shape")
    cosw = torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30)
    w = math.acos(float(cosw.clamp(-1.0, 1.0)))
    t = torch.linspace(0.0, 1.0, steps, dtype=torch.float64).view(-1, 1)
    if math.sin(w) < 1e-6:
        out = (1.0 - t) * a + t * b
    else:
        out = (torch.sin((1.0 - t) * w) * a + torch.sin(t * w) * b) / math.sin(w)
    out[0], out[-1] = a, b
    return out.to(z0.dtype).view(steps, *z0.shape)


def one_hot(classes):
    """int class ids [n] -> the one-hot int64 [n,100] labels the CGAN generator takes."""
    c = torch.as_tensor(classes, dtype=torch.int64).view(-1)
    if c.numel() and (int(c.min()) < 0 or int(c.max()) >= N_CLASS):
        raise JckError(f"class ids must lie in [0, {N_CLASS})")
    return torch.nn.functional.one_hot(c, N_CLASS).to(torch.int64)


def images_to_target(images):
    """What a projection fits: uint8 NHWC [n,S,S,3] (as Sampler.images returns and generate.py stores) -> u8 / 127.5 - 1, or fp32
    NCHW [n,3,S,S] in [-1, 1] as it is -> fp32 NCHW [n,3,S,S], S in (64, 128)."""
    x = torch.as_tensor(images)
    if x.dim() != 4:
        raise JckError(f"images must be uint8 [n,S,S,3] or float [n,3,S,S], got shape {tuple(x.shape)}")
    if x.dtype == torch.uint8:
        if x.shape[3] != 3 or x.shape[1] != x.shape[2]:
            raise JckError(f"uint8 images must be NHWC [n,S,S,3], got {tuple(x.shape)}")
        x = (x.to(torch.float32) / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()
    elif x.is_floating_point():
        if x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise JckError(f"float images must be NCHW [n,3,S,S], got {tuple(x.shape)}")
        x = x.to(torch.float32)
    else:
        raise JckError(f"images must be uint8 or floating point, got {x.dtype}")
    if x.shape[0] < 1 or x.shape[2] not in (64, 128):
        raise JckError(f"images must be a non-empty batch of 64x64 or 128x128 pictures, got {tuple(x.shape)}")
    return x


def load_projection_targets(path):
    """The `images` array of an .npz (generate.py's images.npz, or any uint8 [n,S,S,3]) -> (uint8 tensor, labels or None)."""
    import numpy as np
    with np.load(path) as f:
        if "images" not in f.files:
            raise JckError(f"{path}: no 'images' array (found {sorted(f.files)})")
        im = f["images"]
        labels = f["labels"] if "labels" in f.files else None
    if im.dtype != np.uint8 or im.ndim != 4 or im.shape[3] != 3 or im.shape[1] != im.shape[2] or im.shape[0] < 1:
        raise JckError(f"{path}: 'images' must be uint8 [n,S,S,3], got {im.dtype} {tuple(im.shape)}")
    if im.shape[1] not in (64, 128):
        raise JckError(f"{path}: images are {im.shape[1]}x{im.shape[2]}; 64x64 or 128x128 expected")
    if labels is not None and labels.shape[0] != im.shape[0]:
        raise JckError(f"{path}: {labels.shape[0]} labels for {im.shape[0]} images")
    return torch.from_numpy(im.copy()), None if labels is None else torch.from_numpy(labels.copy())


class Sampler:
    def __init__(self, engine, which):
        self.engine, self.which = engine, which
        self.conditional = engine.family == 1

    @classmethod
    def from_checkpoint(cls, path, model="DCGAN", which="auto", prec="bf16", batch=64, device="cuda:0"):
        """path: a file written by the trainers' save_model (or the reference's), or the dict itself."""
        if model not in ("DCGAN", "CGAN"):
            raise JckError(f"model must be 'DCGAN' or 'CGAN', got {model!r}")
        if not torch.cuda.is_available():
            raise JckError("Sampler needs a GPU: the HIP path has no CPU fallback")
        from .engine import CganEngine, DcganEngine
        ckpt = path if isinstance(path, dict) else torch.load(path, map_location="cpu", weights_only=False)
        g_state, picked = pick_generator_state(ckpt, which)
        size = image_size_of(g_state)
        kw = {"image_size": size} if size != 64 else {}
        eng = (CganEngine if model == "CGAN" else DcganEngine)(batch=batch, prec=prec, device=device, **kw)
        eng.load_state(g_state, {})            # the chosen generator is this engine's generator; its D stays unset and unused
        return cls(eng, picked)

    def _labels(self, labels, n):
        if not self.conditional:
            return None
        if labels is None:
            raise JckError("a CGAN sampler needs labels (class ids [n] or one-hot [n,100])")
        lab = torch.as_tensor(labels)
        lab = one_hot(lab) if lab.dim() == 1 else lab.to(torch.int64)
        if lab.shape != (n, N_CLASS):
            raise JckError(f"labels must be [{n}] class ids or [{n},{N_CLASS}] one-hot, got {tuple(lab.shape)}")
        return lab

    def from_latents(self, z, labels=None, bn="running", out="uint8"):
        """bn="batch": z is cut into chunks of the engine's batch, each ONE train-mode BatchNorm batch (the trainers' evaluation
        sampling; the running statistics move, and an image depends on the z of its chunk).  bn="running": the engine chunks."""
        z = z.reshape(-1, NZ)
        lab = self._labels(labels, z.shape[0])
        if bn != "batch" or z.shape[0] <= self.engine.batch:
            return self.engine.sample(z, lab, bn=bn, out=out)
        from .engine import chunk_plan
        return torch.cat([self.engine.sample(z[lo:hi], None if lab is None else lab[lo:hi], bn=bn, out=out)
                          for lo, hi in chunk_plan(z.shape[0], self.engine.batch)])

    def images(self, n, seed=0, truncation=None, labels=None, bn="running", out="uint8"):
        """n images from z = latents(n, seed, truncation): uint8 [n,S,S,3] or fp32 [n,3,S,S] on the device."""
        return self.from_latents(latents(n, seed, truncation), labels, bn, out)

    def interpolate(self, z0, z1, steps, labels=None, bn="running", out="uint8"):
        return self.from_latents(slerp(z0.reshape(NZ), z1.reshape(NZ), steps).float(), labels, bn, out)

    def project(self, images, labels=None, steps=200, lr=0.05, prior=0.0, seed=0, restarts=1, z0=None):
        """The latent z whose image is closest to each of `images` (uint8 NHWC [n,S,S,3] or fp32 NCHW in [-1, 1]): `steps` Adam
        updates through the frozen eval-mode generator (DcganEngine.project) -> (z [n,100], final loss [n]: mean squared error of
        G(z) at the returned z).  restarts=R starts every image from R seeds (seed, seed + 1, ...; run as extra rows) and keeps
        the start that ends lowest."""
        t = images_to_target(images)
        n, R = t.shape[0], int(restarts)
        if t.shape[2] != self.engine.size:
            raise JckError(f"images are {t.shape[2]}x{t.shape[2]}, the generator makes {self.engine.size}x{self.engine.size}")
        if R < 1:
            raise JckError(f"restarts must be >= 1, got {restarts}")
        if z0 is not None and R != 1:
            raise JckError("z0 fixes the start: restarts must be 1")
        lab = self._labels(labels, n)
        t = t.to(self.engine.device)
        tt = t.repeat(R, 1, 1, 1) if R > 1 else t                     # row r * n + i: image i from seed + r
        ll = None if lab is None else lab.repeat(R, 1)
        if z0 is None:
            z0 = torch.cat([latents(n, int(seed) + r) for r in range(R)])
        z, _ = self.engine.project(tt, ll, steps=steps, lr=lr, prior=prior, z0=z0.reshape(-1, NZ))
        loss, _ = self.engine.latent_grad(z, tt, ll)
        if R > 1:
            best = loss.view(R, n).argmin(0)                            # ties: the lowest seed
            pick = best * n + torch.arange(n, device=best.device)
            z, loss = z[pick], loss[pick]
        return z, loss

    def calibrate(self, batches, seed=0):
        """`batches` train-mode sampling batches (full engine batches of fresh z, uniform random classes for a CGAN) through the
        training-schedule path, so that the running statistics (momentum 0.1 each) belong to the weights being sampled."""
        b = self.engine.batch
        g = torch.Generator().manual_seed(int(seed))
        for _ in range(int(batches)):
            z = torch.randn(b, NZ, generator=g)
            lab = one_hot(torch.randint(0, N_CLASS, (b,), generator=g)) if self.conditional else None
            self.engine.sample(z, lab)
