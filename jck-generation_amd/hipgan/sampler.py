"""Generator inference outside the trainer: load a checkpoint's generator into a step engine of its own and draw images.

    s = Sampler.from_checkpoint("best.pt", "DCGAN")          # the averaged generator when the file has one
    u8 = s.images(1000, seed=0, truncation=0.7)                # uint8 [1000,S,S,3] on the device
    r = s.neighbours(u8, train_u8, k=4)                        # nearest training images: r["idx"], r["rmse"], r["copy"]
    s = Sampler.from_checkpoint("best.pt", "DCGAN", with_d=True)   # ... with the checkpoint's discriminator
    r = s.inpaint(u8, parse_mask("center:32", 64))             # hipgan.inpaint: z fitted to the known pixels, D as realism prior
    z2, before, after = s.refine(z, steps=10)                  # latents moved along the discriminator's gradient
    f = s.features(u8)                                         # D's pooled conv activations, fp32 [n,15360] (hipgan.probe)
    r = s.knn_probe(train_u8, train_labels, test_u8, test_labels)    # what D learned about the classes: r["accuracy"]
    c = s.cluster(train_u8, 100)                               # k-means of the training set on D's features: c["labels"], c["centres"]
    m = s.modes(train_u8, n=10000, k=100)                      # mode coverage (hipgan.cluster): m["covered"], m["kl"], m["missing"]
    v = s.diversity(2000, pairs=1000, train_u8=train_u8)       # mean MS-SSIM of random pairs against the training set's (hipgan.diversity)
    w = s.swd(train_u8, n=8192)                                # sliced Wasserstein distance per pyramid level (hipgan.swd): w["swd"], w["mean"]
    f = s.spectrum(train_u8, n=8192)                           # power spectra against the training set's (hipgan.spectrum): f["gap_db"], f["checkerboard_db"]

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


def pick_discriminator_state(ckpt):
    """The discriminator state dict of a checkpoint dict ('model_d')."""
    if not isinstance(ckpt, dict) or "model_d" not in ckpt:
        raise JckError("checkpoint has no 'model_d' entry: scoring and score-guided sampling need the trained discriminator")
    d = ckpt["model_d"]
    if not isinstance(d, dict) or not d:
        raise JckError("checkpoint's 'model_d' is empty: scoring and score-guided sampling need the trained discriminator")
    return d


def _f64(x):
    """a flat fp64 host copy (Python numbers are taken as fp64, not rounded to the default fp32)"""
    t = x.detach().double() if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float64)
    return t.reshape(-1).cpu()


def select_top(logits, keep):
    """Indices (int64 [keep], best first) of the `keep` largest logits; ties go to the lower index, NaN is never selected."""
    l = _f64(logits)
    keep = int(keep)
    if keep < 0:
        raise JckError(f"select_top: keep must be >= 0, got {keep}")
    ok = ~torch.isnan(l)
    finite = int(ok.sum())
    if finite < keep:
        raise JckError(f"select_top: {keep} wanted, only {finite} of {l.numel()} logits are numbers")
    key = torch.where(ok, l, torch.full_like(l, -math.inf))
    order = torch.sort(key, descending=True, stable=True).indices      # stable: equal logits keep their index order
    order = order[ok[order]]                                            # (a -inf logit is a number; a NaN sorted beside it is not)
    return order[:keep]


def drs_f(logits, max_logit, gamma, eps=1e-8):
    """F of discriminator rejection sampling (Azadi et al. 2019, eq. 8) in fp64:
    F = (l - M) - log(1 - exp(l - M - eps)) - gamma, l clamped to M; NaN stays NaN."""
    l = _f64(logits)
    d = torch.clamp(l - float(max_logit), max=0.0)                      # (clamp passes NaN)
    return d - torch.log(1.0 - torch.exp(d - float(eps))) - float(gamma)


def drs_accept(logits, max_logit, gamma, u, eps=1e-8):
    """bool [n]: sample i is accepted where u[i] < sigmoid(F_i) (drs_f); a NaN logit is rejected."""
    f = drs_f(logits, max_logit, gamma, eps)
    uu = _f64(u)
    if uu.shape != f.shape:
        raise JckError(f"drs_accept: {uu.numel()} uniforms for {f.numel()} logits")
    return (uu < torch.sigmoid(f)) & ~torch.isnan(f)


def image_size_of(g_state):
    """64 for the reference's five-layer generator, 128 for the six-layer plan."""
    n = sum(1 for k in g_state if k.startswith("conv") and k.endswith(".weight"))
    if n not in (5, 6):
        raise JckError(f"generator state has {n} conv layers; 5 (64x64) or 6 (128x128) expected")
    return 64 if n == 5 else 128


def latents(n, seed, truncation=None, generator=None):
    """z [n,100] fp32 on the host from a seeded torch.Generator; truncation t: a standard normal truncated to [-t, t]
    (torch.nn.init.trunc_normal_).  generator: continue this stream instead of starting one from `seed`."""
    g = torch.Generator().manual_seed(int(seed)) if generator is None else generator
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


def fit_images(images, size, what):
    """images_to_target(images), refused unless they are `size` x `size`: what an engine's generator makes and its discriminator takes"""
    x = images_to_target(images)
    if x.shape[2] != size:
        raise JckError(f"{what}: images are {x.shape[2]}x{x.shape[2]}, this engine's networks are {size}x{size}")
    return x


def restart_rows(n, restarts, seed, *rows):
    """R = restarts starts per image, run as extra rows: (z0 [R*n,100], whose block r is latents(n, seed + r), then every tensor of
    `rows` ([n,...] or None) tiled R times) - row r * n + i is image i from seed + r"""
    z0 = torch.cat([latents(n, int(seed) + r) for r in range(restarts)])
    return (z0,) + tuple(a if a is None or restarts == 1 else a.repeat(restarts, *([1] * (a.dim() - 1))) for a in rows)


def pick_best(score, n, *rows):
    """`rows` ([R*n,...] each, laid out as restart_rows leaves them) cut to the start with the lowest score [R*n] per image: [n,...]
    each.  Ties go to the lowest seed; R = 1 returns the rows as they are."""
    if score.shape[0] == n:
        return rows
    best = score.view(-1, n).argmin(0)                                  # the first minimum: the lowest seed
    pick = best * n + torch.arange(n, device=best.device)
    return tuple(a[pick] for a in rows)


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
    def from_checkpoint(cls, path, model="DCGAN", which="auto", prec="bf16", batch=64, device="cuda:0", with_d=False):
        """path: a file written by the trainers' save_model (or the reference's), or the dict itself.
        with_d: load the checkpoint's discriminator too ('model_d'), for score() and images(select=...)."""
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
        d_state = pick_discriminator_state(ckpt) if with_d else {}
        if with_d:
            kind = "CGAN" if "linear1.weight" in d_state else "DCGAN"
            if kind != model:
                raise JckError(f"checkpoint's 'model_d' is a {kind} discriminator, the sampler was asked for {model}")
        eng.load_state(g_state, d_state)       # the chosen generator is this engine's generator; without with_d its D stays unset
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
        from .engine_infer import chunk_plan
        return torch.cat([self.engine.sample(z[lo:hi], None if lab is None else lab[lo:hi], bn=bn, out=out)
                          for lo, hi in chunk_plan(z.shape[0], self.engine.batch)])

    def images(self, n, seed=0, truncation=None, labels=None, bn="running", out="uint8", select=None, oversample=4,
               gamma_percentile=80.0, return_info=False, refine_steps=10, refine_lr=0.02):
        """n images from z = latents(n, seed, truncation): uint8 [n,S,S,3] or fp32 [n,3,S,S] on the device.

        select (needs the discriminator: from_checkpoint(..., with_d=True); eval-mode BatchNorm; labels: None or ONE class id / one-hot
        row for all draws of a CGAN): "top" draws oversample * n latents from the seeded stream and keeps the n the discriminator
        scores highest (best first); "drs" is discriminator rejection sampling (Azadi et al. 2019): one burn-in draw of oversample * n
        fixes M (its largest logit) and gamma (the gamma_percentile-th percentile of F at gamma = 0), then rounds of oversample * n
        latents and uniforms from the same seeded generator are accepted where u < sigmoid(F) until n are kept - at most 50 * n
        draws after the burn-in, JckError beyond.  Deterministic for a seed.
        "refine" draws n latents and moves each along the discriminator's gradient (refine_steps Adam updates at refine_lr on -logit,
        DcganEngine.refine): the images are those of the refined latents, info holds "logit_before" and "logit_after" too.
        return_info: (images, {"z": [n,100], "logit": [n], "prob": [n], "drawn": latents drawn, "max_logit", "gamma"})."""
        if select == "refine":
            if bn != "running":
                raise JckError("refinement follows the eval-mode discriminator's gradient: bn must be 'running'")
            img, info = self._images_refine(int(n), seed, truncation, labels, out, refine_steps, refine_lr)
            return (img, info) if return_info else img
        if select is None:
            z = latents(n, seed, truncation)
            img = self.from_latents(z, labels, bn, out)
            return (img, {"z": z, "logit": None, "prob": None, "drawn": n}) if return_info else img
        if select not in ("top", "drs"):
            raise JckError(f"select must be None, 'top', 'drs' or 'refine', got {select!r}")
        if bn != "running":
            raise JckError("score-guided sampling scores the eval-mode generator: bn must be 'running'")
        n, m = int(n), int(oversample)
        if n < 1 or m < 1:
            raise JckError(f"select={select!r}: n >= 1 and oversample >= 1, got {n}, {oversample}")
        if not 0.0 <= float(gamma_percentile) <= 100.0:
            raise JckError(f"gamma_percentile must lie in [0, 100], got {gamma_percentile}")
        if select == "drs" and m > 50:
            raise JckError(f"select='drs': oversample {m} exceeds the cap of 50 * n draws in its first round; use oversample <= 50")
        g = torch.Generator().manual_seed(int(seed))                        # ONE seeded stream: latents, then uniforms, per round
        info = self._images_top(n, m, g, truncation, labels) if select == "top" else self._images_drs(n, m, g, truncation, labels, gamma_percentile)
        img = self.from_latents(info["z"], self._one_class(labels, n), "running", out)
        return (img, info) if return_info else img

    def _one_class(self, labels, k):
        """one-hot [k,100] of the ONE class (an id or a one-hot row) all k draws of a score-guided CGAN run share; None for a DCGAN"""
        if not self.conditional:
            return None
        if labels is None:
            raise JckError("a CGAN sampler needs labels (one class id or one one-hot row for score-guided sampling)")
        lab = torch.as_tensor(labels)
        lab = one_hot(lab.view(-1)) if lab.dim() <= 1 else lab.to(torch.int64)
        if lab.shape != (1, N_CLASS):
            raise JckError("score-guided sampling of a CGAN takes ONE class (an id or a [1,100] one-hot row)")
        return lab.expand(k, N_CLASS).contiguous()

    def _images_refine(self, n, seed, truncation, labels, out, steps, lr):
        z0 = latents(n, seed, truncation)
        lab = self._labels(labels, n)
        z, before, after = self.refine(z0, lab, steps=steps, lr=lr)
        img = self.engine.sample(z, lab, bn="running", out=out)
        return img, {"z": z.cpu(), "logit": after.cpu(), "prob": torch.sigmoid(after).cpu(), "drawn": n, "logit_before": before.cpu(),
                     "logit_after": after.cpu()}

    def _images_top(self, n, m, g, truncation, labels):
        """the n best of m * n draws of the stream g, best first -> info"""
        z = latents(m * n, 0, truncation, generator=g)
        logit, prob = (t.cpu() for t in self.engine.score_latents(z, self._one_class(labels, m * n)))
        idx = select_top(logit, n)
        return {"z": z[idx], "logit": logit[idx], "prob": prob[idx], "drawn": m * n}

    def _images_drs(self, n, m, g, truncation, labels, gamma_percentile):
        """discriminator rejection sampling: a burn-in of m * n draws of the stream g fixes M and gamma, then rounds of m * n latents
        and as many uniforms are accepted where u < sigmoid(F) until n are kept -> info"""
        lab = self._one_class(labels, m * n)
        burn = self.engine.score_latents(latents(m * n, 0, truncation, generator=g), lab)[0].cpu()
        finite = burn[~torch.isnan(burn)].double()
        if finite.numel() == 0:
            raise JckError("select='drs': every burn-in logit is NaN")
        M = float(finite.max())
        gamma = float(torch.quantile(drs_f(finite, M, 0.0), float(gamma_percentile) / 100.0))
        zs, ls, ps, drawn, kept = [], [], [], 0, 0
        while kept < n:
            if drawn + m * n > 50 * n:
                raise JckError(f"select='drs': {kept} of {n} accepted after {drawn} draws (cap 50 * n); lower gamma_percentile")
            z = latents(m * n, 0, truncation, generator=g)
            u = torch.rand(m * n, generator=g, dtype=torch.float64)
            logit, prob = (t.cpu() for t in self.engine.score_latents(z, lab))
            acc = drs_accept(logit, M, gamma, u)
            zs.append(z[acc]); ls.append(logit[acc]); ps.append(prob[acc])
            drawn += m * n
            kept += int(acc.sum())
        return {"max_logit": M, "gamma": gamma, "burn_in": m * n, "z": torch.cat(zs)[:n], "logit": torch.cat(ls)[:n], "prob": torch.cat(ps)[:n],
                "drawn": drawn}

    def from_latents_scored(self, z, labels=None, out="uint8"):
        """(images, logit [n], prob [n]): the eval-mode generator's images of z and the discriminator's scores of exactly those
        images, each chunk scored where the generator left it - G runs once."""
        z = z.reshape(-1, NZ)
        return self.engine.sample_scored(z, self._labels(labels, z.shape[0]), out=out)

    def score(self, images, labels=None):
        """(logit [n], prob [n]) on the device: the checkpoint's discriminator under model.eval() on uint8 NHWC or fp32 NCHW images
        (DcganEngine.score).  Needs from_checkpoint(..., with_d=True)."""
        n = torch.as_tensor(images).shape[0]
        return self.engine.score(images, self._labels(labels, n))

    def score_latents(self, z, labels=None):
        """(logit [n], prob [n]) of D(G(z)), both networks in eval mode, the images never leaving the device."""
        z = z.reshape(-1, NZ)
        return self.engine.score_latents(z, self._labels(labels, z.shape[0]))

    def interpolate(self, z0, z1, steps, labels=None, bn="running", out="uint8"):
        return self.from_latents(slerp(z0.reshape(NZ), z1.reshape(NZ), steps).float(), labels, bn, out)

    def project(self, images, labels=None, steps=200, lr=0.05, prior=0.0, seed=0, restarts=1, z0=None, feature_weight=0.0,
                feature_stage=None):
        """The latent z whose image is closest to each of `images` (uint8 NHWC [n,S,S,3] or fp32 NCHW in [-1, 1]): `steps` Adam
        updates through the frozen eval-mode generator (DcganEngine.project) -> (z [n,100], final loss [n]: mean squared error of
        G(z) at the returned z).  restarts=R starts every image from R seeds (seed, seed + 1, ...; run as extra rows) and keeps
        the start that ends lowest.
        feature_weight > 0 (perceptual projection; needs from_checkpoint(..., with_d=True)): feature_weight * the mean squared
        distance between the discriminator's stage-`feature_stage` activations (None: the deepest) of G(z) and of the image joins
        the objective (DcganEngine.project(feature_target=images)); the loss returned and compared stays the pixel error."""
        fw = float(feature_weight)
        if not (fw >= 0.0 and fw < float("inf")):
            raise JckError(f"project: feature_weight must be finite and >= 0, got {feature_weight}")
        if fw > 0.0:
            self._needs_d("project(feature_weight > 0)")
        t, n, R = self._targets("project", images, restarts)
        if z0 is not None and R != 1:
            raise JckError("z0 fixes the start: restarts must be 1")
        zr, tt, ll = restart_rows(n, R, seed, t, self._labels(labels, n))
        feat = dict(feature_target=tt, feature_weight=fw, feature_stage=feature_stage) if fw > 0.0 else {}
        z, _ = self.engine.project(tt, ll, steps=steps, lr=lr, prior=prior, z0=(zr if z0 is None else z0).reshape(-1, NZ), **feat)
        loss, _ = self.engine.latent_grad(z, tt, ll)
        return pick_best(loss, n, z, loss)

    def _targets(self, what, images, restarts):
        """(the images as fp32 NCHW on the engine's device, n, R) of a call that fits latents to images from R = restarts starts each"""
        t = fit_images(images, self.engine.size, what)
        if int(restarts) < 1:
            raise JckError(f"{what}: restarts must be >= 1, got {restarts}")
        return t.to(self.engine.device), t.shape[0], int(restarts)

    def _needs_d(self, what):
        if not self.engine._shared.get("d_loaded"):
            raise JckError(f"{what}: the critic is this checkpoint's discriminator: Sampler.from_checkpoint(..., with_d=True)")

    def refine(self, z, labels=None, steps=10, lr=0.02, mode="logit", prior=0.0):
        """(z' [n,100], logit_before [n], logit_after [n]) on the device: `steps` Adam updates of each latent along the eval-mode
        discriminator's gradient (DcganEngine.refine).  Needs from_checkpoint(..., with_d=True)."""
        self._needs_d("refine")
        z = z.reshape(-1, NZ)
        return self.engine.refine(z, self._labels(labels, z.shape[0]), steps=steps, lr=lr, mode=mode, prior=prior)

    def inpaint(self, images_u8, known, labels=None, steps=300, lr=0.05, critic_weight=0.003, window=7, restarts=1, seed=0):
        """Semantic inpainting (Yeh et al. 2017): fits z to the KNOWN pixels of `images_u8` (uint8 NHWC [n,S,S,3]; known: bool [S,S]
        or [n,S,S], hipgan.inpaint.parse_mask) with the importance weighting of `window` (hipgan.inpaint.importance_weights) and
        critic_weight * -log D(G(z)) as the realism prior (0: none, and no discriminator is needed).
        -> {"z" [n,100], "loss" [n] (weighted, at z), "term" [n], "generated" uint8 [n,S,S,3] = G(z), "completed" uint8: the known
        pixels of the input, the holes from G}.  restarts=R: R seeds per image, the one ending at the lowest loss + term kept."""
        from .inpaint import _check_known, blend, importance_weights
        x = torch.as_tensor(images_u8)
        if x.dtype != torch.uint8:
            raise JckError(f"inpaint: images must be uint8 [n,S,S,3], got {x.dtype}")
        t, n, R = self._targets("inpaint", x, restarts)
        k = _check_known(torch.as_tensor(known).cpu(), self.engine.size, "inpaint")
        if k.dim() == 3 and k.shape[0] != n:
            raise JckError(f"inpaint: {k.shape[0]} masks for {n} images")
        cw = float(critic_weight)
        if not cw >= 0.0:
            raise JckError(f"inpaint: critic_weight must be >= 0, got {critic_weight}")
        critic = "nsgan" if cw > 0.0 else None
        if critic:
            self._needs_d("inpaint")
        w = importance_weights(k, window)
        w = w if w.dim() == 3 else w.unsqueeze(0).expand(n, -1, -1)
        if bool((w.reshape(n, -1).sum(1) <= 0).any()):
            raise JckError("inpaint: the importance weights of an image are all zero (no known pixel has a hole within the window)")
        lab = self._labels(labels, n)
        z0, tt, ww, ll = restart_rows(n, R, seed, t, w.contiguous(), lab)
        z, _ = self.engine.project(tt, ll, steps=steps, lr=lr, z0=z0, weight=ww, critic=critic, critic_weight=cw)
        res = self.engine.latent_grad(z, tt, ll, weight=ww, critic=critic, critic_weight=cw)
        loss, term = (res[0], res[1]) if critic else (res[0], torch.zeros_like(res[0]))
        z, loss, term = pick_best(loss + term if R > 1 else loss, n, z, loss, term)      # (one start: nothing to add up for)
        gen = self.engine.sample(z, lab, bn="running", out="uint8")
        return {"z": z, "loss": loss, "term": term, "generated": gen, "completed": blend(x.to(gen.device), gen, k)}

    def anomaly(self, images, labels=None, steps=300, lr=0.05, lam=0.1, stage=None, restarts=1, seed=0):
        """Anomaly scores after AnoGAN (Schlegl et al. 2017): every image (uint8 NHWC [n,S,S,3] or fp32 NCHW in [-1, 1]) is projected
        onto the generator with a residual term R = L (the mean squared pixel error) and a feature-matching term D = F_unit (the mean
        squared distance between the discriminator's stage-`stage` activations of G(z) and of the image; None: the deepest stage),
        and scored by what remains: score = (1 - lam) R + lam D (hipgan.anomaly.anomaly_score).  `steps` Adam updates minimise
        L + lam / (1 - lam) * F_unit, which has the minimiser of (1 - lam) R + lam D; one more evaluation at the final z gives the
        numbers.  -> {"z" [n,100], "residual" [n] = L, "feature" [n] = F / feat_weight, "score" [n] (fp64), "generated" uint8 = G(z)}.
        restarts=R: R seeds per image (seed, seed + 1, ...), the one ending at the lowest score kept.
        R and D here are the mean squared forms of this code base's losses, not AnoGAN's L1 sums, so scores are not comparable with
        the paper's numbers; and whether the discriminator's features separate anything is a property of the run that trained it.
        Needs from_checkpoint(..., with_d=True)."""
        from .anomaly import anomaly_score
        lam = float(lam)
        if not 0.0 <= lam < 1.0:
            raise JckError(f"anomaly: lam must lie in [0, 1), got {lam}")
        t, n, R = self._targets("anomaly", images, restarts)
        self._needs_d("anomaly")
        lab = self._labels(labels, n)
        z0, tt, ll = restart_rows(n, R, seed, t, lab)
        fw = lam / (1.0 - lam)
        if fw > 0.0:
            feat = dict(feature_target=tt, feature_weight=fw, feature_stage=stage)
            z, _ = self.engine.project(tt, ll, steps=steps, lr=lr, z0=z0, **feat)
            res = self.engine.latent_grad(z, tt, ll, **feat)
            residual, feature = res["loss"], res["fterm"] / fw
        else:                                                            # lam = 0: the residual alone decides; D is still reported
            z, _ = self.engine.project(tt, ll, steps=steps, lr=lr, z0=z0)
            residual = self.engine.latent_grad(z, tt, ll)[0]
            feature = self.engine.latent_grad(z, tt, ll, feature_target=tt, feature_weight=1.0, feature_stage=stage)["fterm"]
        score = anomaly_score(residual, feature, lam)
        z, residual, feature, score = pick_best(score, n, z, residual, feature, score)
        gen = self.engine.sample(z, lab, bn="running", out="uint8")
        return {"z": z, "residual": residual, "feature": feature, "score": score, "generated": gen}

    def neighbours(self, images, ref, k=4, space="pixel", grid=4, pool="max", normalise="block", **kw):
        """The k nearest reference (training) images of `images`, both uint8 NHWC, and the `copy` flags, on this sampler's device.
        space="pixel": in pixel space (hipgan.neighbours.nearest_images).  space="d": the same walk on the discriminator's
        block-normalised features (hipgan.probe.extract with grid, pool, normalise; needs from_checkpoint(..., with_d=True)), which
        also finds a shifted, recoloured or mirrored picture: idx, d2, ref_nn_d2 and copy, no rmse."""
        if space not in ("pixel", "d"):
            raise JckError(f"neighbours: space must be 'pixel' or 'd', got {space!r}")
        if space == "pixel":
            from .neighbours import nearest_images
            return nearest_images(images, ref, k=k, device=self.engine.device, **kw)
        from .neighbours import nearest_rows
        from .probe import extract
        self._needs_d("neighbours(space='d')")
        q = extract(self.engine, images, grid, pool, normalise)
        return nearest_rows(q, extract(self.engine, ref, grid, pool, normalise), k=k, **kw)

    def features(self, images, grid=4, pool="max"):
        """fp32 [n, F] on the device: the checkpoint's discriminator as a feature extractor on uint8 NHWC or fp32 NCHW images
        (DcganEngine.features; hipgan.probe.feature_layout names the columns).  Needs from_checkpoint(..., with_d=True)."""
        self._needs_d("features")
        return self.engine.features(images, grid=grid, pool=pool)

    def knn_probe(self, train_u8, train_labels, test_u8, test_labels, **kw):
        """A k-nearest-neighbour classifier on the discriminator's features (hipgan.probe.knn_probe): what D has learned about the
        classes.  Needs from_checkpoint(..., with_d=True)."""
        from .probe import knn_probe
        self._needs_d("knn_probe")
        return knn_probe(self.engine, train_u8, train_labels, test_u8, test_labels, **kw)

    def _cluster_rows(self, images_u8, space, grid, pool, what):
        """fp32 [n,D] on the device, the rows a clustering works on: space="d": the discriminator's block-normalised features
        (hipgan.probe.extract); space="pixel": u8 / 127.5 - 1 flattened, 32 x 32 data upscaled as `neighbours` does"""
        if space not in ("pixel", "d"):
            raise JckError(f"{what}: space must be 'pixel' or 'd', got {space!r}")
        if space == "d":
            from .probe import extract
            self._needs_d(f"{what}(space='d')")
            return extract(self.engine, images_u8, grid, pool)
        from .neighbours import _check_u8, _rows, upscale_steps
        x = _check_u8(images_u8, "images")
        return _rows(x, upscale_steps(x.shape[1], self.engine.size, "training"), self.engine.device)

    def cluster(self, train_u8, k, space="d", seed=0, iters=50, grid=4, pool="max"):
        """k-means (hipgan.cluster.kmeans, on the device) of the training pictures (uint8 NHWC) in the discriminator's block-normalised
        feature space (space="d"; grid, pool as hipgan.probe.extract takes them; needs from_checkpoint(..., with_d=True)) or in pixel
        space -> kmeans' dict of device tensors: "centres" [k,D], "labels" [N], "count" [k], "d2", "inertia", "iters", "history".
        "labels" are the usual pseudo-labels of unlabelled pictures."""
        from .cluster import kmeans
        return kmeans(self._cluster_rows(train_u8, space, grid, pool, "cluster"), k, iters=iters, seed=seed)

    def modes(self, train_u8, n=10000, k=100, seed=0, truncation=None, labels=None, clusters=None, min_count=1, space="d", grid=4,
              pool="max", **cluster_kw):
        """Mode coverage: did the generator collapse?  The training pictures are clustered (cluster(train_u8, k, space, seed, grid=, pool=,
        **cluster_kw), unless `clusters` is a dict from cluster() in the same space), n images are drawn from latents(n, seed, truncation)
        with bn="running" (labels: a CGAN's class ids [n] or one-hot rows), a chunk at a time, their rows are made the same way and
        assigned to the nearest centre (metrics.nearest) -> hipgan.cluster.coverage(count, sample clusters, min_count) - "k", "k_real",
        "covered", "expected_covered", "kl", "hist_real", "hist_fake", "missing" - plus, as host arrays, "sample_cluster" int64 [n],
        "sample_d2" fp32 [n], "train_labels" int64 [N], "train_d2" fp32 [N], "centres" fp32 [k,D], "z" fp32 [n,100], and "inertia" and
        "iters" of the clustering."""
        from metrics import nearest
        from .cluster import coverage
        n = int(n)
        if n < 1:
            raise JckError(f"modes: n = {n} must be >= 1")
        cl = clusters if clusters is not None else self.cluster(train_u8, k, space=space, seed=seed, grid=grid, pool=pool, **cluster_kw)
        centres = torch.as_tensor(cl["centres"]).to(device=self.engine.device, dtype=torch.float32).contiguous()
        z = latents(n, seed, truncation)
        lab = self._labels(labels, n)
        step = max(self.engine.batch, 1024)
        which, dist = [], []
        for lo in range(0, n, step):
            u8 = self.from_latents(z[lo:lo + step], None if lab is None else lab[lo:lo + step])
            rows = self._cluster_rows(u8, space, grid, pool, "modes")
            if rows.shape[1] != centres.shape[1]:
                raise JckError(f"modes: the clusters' centres have {centres.shape[1]} columns, the samples' rows {rows.shape[1]}")
            idx, d2 = nearest(rows, centres, 1)
            which.append(idx[:, 0].cpu())
            dist.append(d2[:, 0].cpu())
        which, dist = torch.cat(which).numpy(), torch.cat(dist).numpy()
        host = lambda v: torch.as_tensor(v).cpu().numpy()
        out = coverage(host(cl["count"]), which, min_count)
        out.update(sample_cluster=which, sample_d2=dist, train_labels=host(cl["labels"]).astype("int64"), train_d2=host(cl["d2"]),
                   centres=host(centres), z=z.numpy(), inertia=float(cl["inertia"]), iters=int(cl["iters"]))
        return out

    def diversity(self, n, pairs=1000, seed=0, labels=None, train_u8=None, train_labels=None, levels=None, truncation=None, top=16):
        """Sample diversity (hipgan.diversity): does every sample (of a class) look the same?  n images are drawn from latents(n, seed,
        truncation) with bn="running" (labels: a CGAN's class ids [n] or one-hot rows), a chunk at a time, and kept as uint8 on the
        device; `pairs` random pairs (per class; draw_pairs(n, pairs, seed, class ids)) go through metrics.ssim_pairs at `levels`
        (None: default_levels of the networks' size).  train_u8 (uint8 NHWC, 32 x 32 data upscaled as the trainers do) with
        train_labels (class ids, for a CGAN) gets the same treatment, and the two are compared class by class ->
          "levels", "images" (uint8 [n,S,S,3], device), "z" fp32 [n,100], "pairs" (draw_pairs' dict), "ssim", "ms_ssim", "sq_err"
          (host arrays [P]), "summary": {"ms_ssim", "ssim": hipgan.diversity.summarise}, "dropped", "top": the indices of the `top`
          pairs with the highest MS-SSIM (near-duplicate samples; ties to the lower pair index), and with training pictures "train":
          the same keys for them (but "images", "z", "top") and "comparison": hipgan.diversity.compare of the two MS-SSIM summaries.
        Without labels all pictures are one class 0."""
        from .diversity import compare, default_levels, pair_diversity, top_pairs
        from .probe import _to_size
        n = int(n)
        if n < 2:
            raise JckError(f"diversity: n = {n} must be >= 2")
        L = default_levels(self.engine.size) if levels is None else int(levels)
        z, lab, u8 = self._draw_u8(n, seed, truncation, labels)
        ids = None if lab is None else lab.argmax(1).numpy()
        out = pair_diversity(u8, pairs, seed, ids, L)
        out.update(levels=L, images=u8, z=z.numpy(), top=top_pairs(out["ms_ssim"], top))
        if train_u8 is not None:
            t = _to_size(train_u8, self.engine.size, "training images").to(self.engine.device).contiguous()
            tl = train_labels if self.conditional else None                  # an unconditional generator has one class, so has its data
            out["train"] = pair_diversity(t, pairs, seed, None if tl is None else torch.as_tensor(tl).cpu().numpy(), L)
            out["comparison"] = compare(out["summary"]["ms_ssim"], out["train"]["summary"]["ms_ssim"])
        return out

    def _draw_u8(self, n, seed, truncation, labels):
        """(z fp32 [n,100], the one-hot labels or None, uint8 [n,S,S,3] on the device): n images from latents(n, seed, truncation) with
        bn="running", drawn a chunk at a time"""
        z = latents(n, seed, truncation)
        lab = self._labels(labels, n)
        step = max(self.engine.batch, 1024)
        u8 = torch.cat([self.from_latents(z[lo:lo + step], None if lab is None else lab[lo:lo + step]) for lo in range(0, n, step)])
        return z, lab, u8

    def _against_training(self, what, train_u8, n, seed, labels, train_labels, truncation, classes, compare):
        """The samples-against-training-set driver of `swd` and `spectrum`: n images from _draw_u8 against the first n training pictures
        (uint8 NHWC, 32 x 32 data upscaled as `neighbours` does) after numpy.random.default_rng(seed).permutation, both uint8 on the
        device.  compare(samples, training pictures) -> the report dict, to which "n", "n_train" and "seed" are added and, with classes
        (ids; needs labels and train_labels), "per_class": {id: compare's dict for the samples and the training pictures of that class,
        as many of each as the smaller side has, "n" among its keys}."""
        import numpy as np

        from .probe import _to_size
        n = int(n)
        if n < 1:
            raise JckError(f"{what}: n = {n} must be >= 1")
        t = _to_size(train_u8, self.engine.size, "training images")
        if t.shape[0] < n:
            raise JckError(f"{what}: {t.shape[0]} training pictures are fewer than the n = {n} samples they are compared with")
        order = np.random.default_rng(int(seed)).permutation(int(t.shape[0]))
        pick = torch.from_numpy(order[:n])
        _, lab, u8 = self._draw_u8(n, seed, truncation, labels)
        out = compare(u8, t[pick].to(self.engine.device).contiguous())
        out.update(n=n, n_train=int(t.shape[0]), seed=int(seed))
        if classes is not None:
            if lab is None or train_labels is None:
                raise JckError(f"{what}: per-class reports need the samples' labels and train_labels")
            ids = lab.argmax(1)
            tl = torch.as_tensor(train_labels).cpu().view(-1).to(torch.int64)[torch.from_numpy(order)]
            out["per_class"] = {}
            for c in classes:
                mine, theirs = torch.nonzero(ids.cpu() == int(c)).view(-1), torch.from_numpy(order)[tl == int(c)]
                k = min(int(mine.shape[0]), int(theirs.shape[0]))
                if k < 1:
                    raise JckError(f"{what}: class {c} has {mine.shape[0]} samples and {theirs.shape[0]} training pictures")
                r = compare(u8[mine[:k].to(u8.device)].contiguous(), t[theirs[:k]].to(self.engine.device).contiguous())
                r.update(n=k)
                out["per_class"][int(c)] = r
        return out

    def swd(self, train_u8, n=8192, seed=0, labels=None, train_labels=None, truncation=None, classes=None, **kw):
        """Sliced Wasserstein distance of the samples' Laplacian-pyramid patch statistics to the training set's, level by level
        (hipgan.swd, metrics.swd; no metric network).  n images are drawn from latents(n, seed, truncation) with bn="running" (labels:
        a CGAN's class ids [n] or one-hot rows), a chunk at a time, and kept as uint8 on the device; of the training pictures (uint8
        NHWC, 32 x 32 data upscaled as `neighbours` does) the first n after numpy.random.default_rng(seed).permutation are taken.  kw
        goes to metrics.swd (levels, patches, dirs, repeats, chunk) -> its dict ("swd" x 1e3 per level, "mean", "sides", "per_repeat")
        plus "n", "n_train", "seed" and, with classes (ids; needs labels and train_labels), "per_class": {id: the same dict for the
        samples and the training pictures of that class, as many of each as the smaller side has, "n" among its keys}."""
        from metrics import swd as metric
        return self._against_training("swd", train_u8, n, seed, labels, train_labels, truncation, classes,
                                      lambda a, b: metric(a, b, seed=seed, **kw))

    def spectrum(self, train_u8, n=8192, seed=0, labels=None, train_labels=None, truncation=None, classes=None, **kw):
        """Power spectra of the samples against the training set's (hipgan.spectrum, metrics.spectrum / spectrum_report):
        the radial profiles' gap in dB per bin, the lattice peaks that stride-2 transposed convolutions leave (checkerboard_db), and
        how well a linear rule on the profile tells the sets apart (separability).  The samples and the training pictures are taken
        exactly as `swd` takes them: n images from latents(n, seed, truncation) with bn="running" (labels: a CGAN's class ids [n] or
        one-hot rows), a chunk at a time, kept as uint8 on the device; the first n training pictures (uint8 NHWC, 32 x 32 data upscaled
        as `neighbours` does) after numpy.random.default_rng(seed).permutation.  kw goes to metrics.spectrum (plane, window, chunk; the
        mean planes are always formed) -> the report dict plus "n", "n_train", "seed" and, with classes (ids; needs labels and
        train_labels), "per_class": {id: the same report for that class's samples and training pictures, as many of each as the smaller
        side has, "n" among its keys}."""
        from metrics import spectrum as metric
        from metrics import spectrum_report
        kw = {**kw, "mean2d": True}
        return self._against_training("spectrum", train_u8, n, seed, labels, train_labels, truncation, classes,
                                      lambda a, b: spectrum_report(metric(a, **kw), metric(b, **kw)))

    def calibrate(self, batches, seed=0):
        """`batches` train-mode sampling batches (full engine batches of fresh z, uniform random classes for a CGAN) through the
        training-schedule path, so that the running statistics (momentum 0.1 each) belong to the weights being sampled."""
        b = self.engine.batch
        g = torch.Generator().manual_seed(int(seed))
        for _ in range(int(batches)):
            z = torch.randn(b, NZ, generator=g)
            lab = one_hot(torch.randint(0, N_CLASS, (b,), generator=g)) if self.conditional else None
            self.engine.sample(z, lab)
