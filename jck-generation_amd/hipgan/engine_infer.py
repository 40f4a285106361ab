"""The engine's inference methods (csrc/engine_infer.hip: jck_engine_sample_ex, _latent_grad_fm, _project_fm, _score, _features), as
the base class of hipgan.engine.DcganEngine, which holds the state and the training step.

Every method here runs both networks as under model.eval() unless it says otherwise, takes any n (rows go through in chunks of at
most `batch`, each row's numbers those of a call with that row alone) and writes nothing of the training state.
"""
import torch

from ._lib import JckError, cur_stream, lib
from .probe import POOL_MODES, feature_layout
from .sampler import fit_images, images_to_target

SAMPLE_EVAL = 1            # include/jckgan.h: JCK_SAMPLE_EVAL
CRITIC_MODES = {None: 0, "nsgan": 1, "logit": 2}      # jck_engine_latent_grad_ex's critic_mode


def _rows(x, lo, hi):
    """rows [lo, hi) of a tensor, None of None"""
    return None if x is None else x[lo:hi]


def chunk_plan(n, batch):
    """[(lo, hi)] covering range(n) in pieces of at most `batch` rows, all but the last full."""
    if n < 0 or batch < 1:
        raise JckError(f"chunk_plan: n >= 0 and batch >= 1, got {n}, {batch}")
    return [(lo, min(lo + batch, n)) for lo in range(0, n, batch)]


class LatentObjective:
    """What a latent call minimises, validated and on the device (EngineInference._objective): the image loss on `target` under the
    per-pixel `weight`, the critic's term (`mode` of CRITIC_MODES at weight `cw`) and the feature-matching term on `feat` at `stage`
    with weight `fw` - the arguments of jck_engine_latent_grad_fm / jck_engine_project_fm.  A tensor that is None is a term that is off."""

    def __init__(self, target, weight, mode, cw, feat, stage, fw):
        self.target, self.weight, self.mode, self.cw, self.feat, self.stage, self.fw = target, weight, mode, cw, feat, stage, fw
        self.tensors = (target, weight, feat)          # for the caller's keep-alive slot: the launches read them after the call returns

    def rows(self, lo, hi):
        """(target, weight, feature target) of the rows [lo, hi)"""
        return _rows(self.target, lo, hi), _rows(self.weight, lo, hi), _rows(self.feat, lo, hi)


class EngineInference:
    def _latents(self, what, z, labels):
        """(n, z as fp32 [n,100] on the device, one-hot int64 labels on the device or None): the latent rows of an inference call"""
        n = z.shape[0]
        if n < 1:
            raise JckError(f"{what}: z is empty")
        zc = z.to(self.device, torch.float32).contiguous().view(-1, 100)
        if zc.shape[0] != n:
            raise JckError(f"{what}: z must be [n,100]")
        return n, zc, self._score_labels(what, labels, n)

    def _image_out(self, n, out):
        """the images of n rows: fp32 NCHW (out="float") or uint8 NHWC (out="uint8")"""
        if out == "uint8":
            return torch.empty(n, self.size, self.size, 3, dtype=torch.uint8, device=self.device)
        return torch.empty(n, 3, self.size, self.size, dtype=torch.float32, device=self.device)

    def _sample_chunk(self, zc, lab, lo, hi, flags, res):
        """rows [lo, hi) through the generator; res (fp32 NCHW, uint8 NHWC or None) receives their images"""
        f32, u8 = (None, None) if res is None else (res[lo:hi], None) if res.dtype == torch.float32 else (None, res[lo:hi])
        lib.jck_engine_sample_ex(self._h, zc[lo:hi], _rows(lab, lo, hi), hi - lo, flags, f32, u8, cur_stream())

    def sample(self, z, labels=None, bn="batch", out="float"):
        """G(z) -> NCHW fp32 [n,3,S,S] on the device (out="float") or NHWC uint8 [n,S,S,3] (out="uint8").

        bn="batch" (the default, train/dcgan_trainer.py:199-200): train-mode BatchNorm.  The whole z is ONE BatchNorm batch
        (statistics and running-stat update over all n samples, as in the reference), so n <= batch and every image depends on
        every z of the call.
        bn="running": the generator as under model.eval() - BatchNorm on its running statistics, folded into the products'
        epilogues.  Every image depends on its own z alone, the buffers do not move, and any n works: z is cut into chunks of
        at most `batch` rows, whose images equal those of separate calls bit for bit."""
        if bn not in ("batch", "running"):
            raise JckError(f"sample: bn must be 'batch' or 'running', got {bn!r}")
        if out not in ("float", "uint8"):
            raise JckError(f"sample: out must be 'float' or 'uint8', got {out!r}")
        n, zc, lab = self._latents("sample", z, labels)
        if bn == "batch" and n > self.batch:
            raise JckError(f"sample: {n} latent vectors exceed this engine's batch {self.batch}; bind an engine with batch >= n "
                           f"(DcganEngine(batch=n, share=engine)), or sample with bn='running', which takes any n")
        self._current()
        res = self._image_out(n, out)
        for lo, hi in chunk_plan(n, self.batch):
            self._sample_chunk(zc, lab, lo, hi, SAMPLE_EVAL if bn == "running" else 0, res)
        self._keep_z = (zc, lab)
        return res

    def _objective(self, what, n, target, weight=None, critic=None, critic_weight=0.0, feature_target=None, feature_weight=0.0,
                   feature_stage=None):
        """The LatentObjective of a latent_grad / critic_grad / project call on n rows, validated on the host: the target (fp32 NCHW
        [n,3,S,S] or None), the feature term (on iff a feature target is given and its weight positive), then the per-pixel weight
        and the critic.  Leaves the engine joined and its operands current, and refuses a critic or a feature term without a
        discriminator."""
        if n < 1:
            raise JckError(f"{what}: no images" if target is not None else f"{what}: no latents")
        if target is not None and (target.dim() != 4 or tuple(target.shape) != (n, 3, self.size, self.size)):
            raise JckError(f"{what}: target must be [{n},3,{self.size},{self.size}] (NCHW, values in [-1, 1]), got {tuple(target.shape)}")
        self._current()
        t = None if target is None else target.to(self.device, torch.float32).contiguous()
        fw = float(feature_weight)
        if not (fw >= 0.0 and fw < float("inf")):
            raise JckError(f"{what}: feature_weight must be finite and >= 0, got {feature_weight}")
        if fw > 0.0 and feature_target is None:
            raise JckError(f"{what}: feature_weight > 0 needs a feature_target")
        ns = len(feature_layout(self.size, 1)[0])
        k = -1 if feature_stage is None else int(feature_stage)
        if not -1 <= k < ns:
            raise JckError(f"{what}: feature_stage must be None / -1 (the deepest) or 0..{ns - 1}, got {feature_stage!r}")
        fx = None
        if feature_target is not None and fw > 0.0:
            fx = images_to_target(feature_target)
            if tuple(fx.shape) != (n, 3, self.size, self.size):
                raise JckError(f"{what}: feature_target must be {n} images of {self.size}x{self.size}, got {tuple(fx.shape)}")
            fx = fx.to(self.device, torch.float32).contiguous()
        if critic not in CRITIC_MODES:
            raise JckError(f"{what}: critic must be None, 'nsgan' or 'logit', got {critic!r}")
        mode, cw = CRITIC_MODES[critic], float(critic_weight)
        if not cw >= 0.0:
            raise JckError(f"{what}: critic_weight must be >= 0, got {critic_weight}")
        if not mode and t is None and fx is None:
            raise JckError(f"{what}: without a target a critic is required")
        w = None
        if weight is not None:
            w = torch.as_tensor(weight)
            if w.dim() == 2:
                w = w.unsqueeze(0).expand(n, -1, -1)
            if tuple(w.shape) != (n, self.size, self.size):
                raise JckError(f"{what}: weight must be [{self.size},{self.size}] or [{n},{self.size},{self.size}], got {tuple(w.shape)}")
            w = w.to(torch.float32)
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise JckError(f"{what}: weights must be finite and >= 0")
            if bool((w.reshape(n, -1).sum(1) <= 0).any()):
                raise JckError(f"{what}: an image's weights are all zero (nothing of it is known)")
            w = w.to(self.device).contiguous()
        if mode or fx is not None:
            self._score_ready(what)
        return LatentObjective(t, w, mode, cw, fx, k, fw if fx is not None else 0.0)

    def _latent_grad(self, zc, lab, o):
        """(loss, term, logit, fterm, dz) of the objective o at the rows of zc: the chunk loop of latent_grad and critic_grad.  Without a
        critic term is 0 and logit NaN, without a feature term fterm is None"""
        n = zc.shape[0]
        f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=self.device)
        loss, dz, fterm = f(n), f(n, 100), None if o.feat is None else f(n)
        term, logit = (f(n), f(n)) if o.mode else (torch.zeros_like(loss), torch.full_like(loss, float("nan")))
        for lo, hi in chunk_plan(n, self.batch):
            t, w, fx = o.rows(lo, hi)
            lib.jck_engine_latent_grad_fm(self._h, zc[lo:hi], _rows(lab, lo, hi), t, w, o.mode, o.cw, hi - lo, loss[lo:hi],
                                          term[lo:hi] if o.mode else None, logit[lo:hi] if o.mode else None, dz[lo:hi], cur_stream(),
                                          fx, o.stage, o.fw, _rows(fterm, lo, hi))
        self._keep_z = (zc, lab) + o.tensors
        return loss, term, logit, fterm, dz

    def latent_grad(self, z, target, labels=None, weight=None, critic=None, critic_weight=0.0, feature_target=None, feature_weight=0.0,
                    feature_stage=None):
        """(loss [n], dz [n,100]): L_b = mean((G(z_b) - target_b)^2) and dL_b/dz_b through the generator as under model.eval()
        (BatchNorm on the running statistics; nothing is written to them).  target: fp32 NCHW [n,3,S,S] in [-1, 1].  Any n: rows
        go through in chunks of at most `batch`, each row's numbers those of a call with that row alone.
        weight ([S,S] or [n,S,S], >= 0): L_b becomes the weighted mean sum_p w_p sum_c (.)^2 / (3 sum_p w_p).  critic ("nsgan" |
        "logit") with critic_weight: the eval-mode discriminator's term critic_weight * c(D(G(z_b))) joins the objective, dz is the
        gradient of the sum and the result is (loss, term [n], logit [n], dz).
        feature_target (fp32 NCHW or uint8 NHWC images) with feature_weight > 0: the feature-matching term F_b = feature_weight *
        mean((a_k(G(z_b)) - a_k(x_b))^2) on the LeakyReLU output of D's conv stage k = feature_stage (None / -1: the deepest) joins
        the objective, target may be None, and the result is the dict {"loss", "term", "logit", "fterm", "dz"} (term 0 and logit NaN
        without a critic)."""
        n, zc, lab = self._latents("latent_grad", z, labels)
        o = self._objective("latent_grad", n, target, weight, critic, critic_weight, feature_target, feature_weight, feature_stage)
        loss, term, logit, fterm, dz = self._latent_grad(zc, lab, o)
        if fterm is not None:
            return {"loss": loss, "term": term, "logit": logit, "fterm": fterm, "dz": dz}
        return (loss, term, logit, dz) if o.mode else (loss, dz)

    def critic_grad(self, z, labels=None, mode="nsgan"):
        """(logit [n], term [n], dz [n,100]): D(G(z)), both networks as under model.eval(), the critic's objective c of it - "nsgan":
        softplus(-logit) = -log D, the generator's training loss; "logit": -logit - and dz = dc/dz.  Any n, rows independent."""
        if mode not in ("nsgan", "logit"):
            raise JckError(f"critic_grad: mode must be 'nsgan' or 'logit', got {mode!r}")
        n, zc, lab = self._latents("critic_grad", z, labels)
        _, term, logit, _, dz = self._latent_grad(zc, lab, self._objective("critic_grad", n, None, critic=mode, critic_weight=1.0))
        return logit, term, dz

    def project(self, target, labels=None, steps=200, lr=0.05, prior=0.0, z0=None, seed=0, state=None, weight=None, critic=None,
                critic_weight=0.0, feature_target=None, feature_weight=0.0, feature_stage=None):
        """Fits z to `target` (fp32 NCHW [n,3,S,S] in [-1, 1]) through the frozen eval-mode generator: `steps` Adam updates
        (lr, betas (0.9, 0.999)) of z minimising mean((G(z) - target)^2) + prior * mean(z^2) per image, all on the device.
        -> (z [n,100], loss_hist [steps,n]: the loss before each update).  z0: the start (default: randn from `seed` on the host);
        state: {"m", "v", "t"} of an earlier call to continue it - the state reached is left in `self.project_state`.
        Any n (chunks of at most `batch` rows; a row's result does not depend on the rows beside it).
        weight / critic / critic_weight: the objective of latent_grad with the same keywords (masked projection: weight 0 on the
        unknown pixels); the critic's term before each update is left in `self.project_term` [steps,n].
        target None (refinement): the critic's term alone.
        feature_target / feature_weight / feature_stage: latent_grad's feature-matching term; it before each update is left in
        `self.project_fterm` [steps,n] (None without the term).  With it the target may be None as well."""
        if target is None and z0 is None:
            raise JckError("project: without a target the start z0 is required")
        n, steps = (z0 if target is None else target).shape[0], int(steps)
        if steps < 1:
            raise JckError(f"project: steps must be >= 1, got {steps}")
        if not float(lr) > 0.0 or float(prior) < 0.0:
            raise JckError(f"project: lr > 0 and prior >= 0, got {lr}, {prior}")
        o = self._objective("project", n, target, weight, critic, critic_weight, feature_target, feature_weight, feature_stage)
        lab = self._score_labels("project", labels, n)
        if z0 is None:
            z0 = torch.randn(n, 100, generator=torch.Generator().manual_seed(int(seed)))
        if tuple(z0.shape) != (n, 100):
            raise JckError(f"project: z0 must be [{n},100], got {tuple(z0.shape)}")
        z = z0.to(self.device, torch.float32).clone().contiguous()
        if state is None:
            m, v, t0 = torch.zeros_like(z), torch.zeros_like(z), 0
        else:
            m, v, t0 = state["m"].to(self.device, torch.float32).clone(), state["v"].to(self.device, torch.float32).clone(), int(state["t"])
            if tuple(m.shape) != (n, 100) or tuple(v.shape) != (n, 100) or t0 < 0:
                raise JckError("project: state must hold m, v [n,100] and t >= 0")
        f = lambda cols: torch.empty(steps, cols, dtype=torch.float32, device=self.device)
        plain = weight is None and critic is None and target is not None
        hist, fterms = f(n), None if o.feat is None else f(n)
        terms = None if plain else torch.zeros(steps, n, dtype=torch.float32, device=self.device)
        for lo, hi in chunk_plan(n, self.batch):
            t, w, fx = o.rows(lo, hi)
            h, th, fh = f(hi - lo), f(hi - lo) if o.mode else None, None if fx is None else f(hi - lo)
            lib.jck_engine_project_fm(self._h, z[lo:hi], _rows(lab, lo, hi), t, hi - lo, steps, float(lr), float(prior), w, o.mode, o.cw,
                                      m[lo:hi], v[lo:hi], t0, h, th, cur_stream(), fx, o.stage, o.fw, fh)
            for whole, part in ((fterms, fh), (terms, th), (hist, h)):
                if part is not None:
                    whole[:, lo:hi] = part
        self._keep_z = (z, lab) + o.tensors
        self.project_state = {"m": m, "v": v, "t": t0 + steps}
        self.project_term = terms
        self.project_fterm = fterms
        return z, hist

    def refine(self, z, labels=None, steps=10, lr=0.02, mode="logit", prior=0.0):
        """Moves latents along the discriminator's gradient: `steps` Adam updates of z minimising the critic's objective alone
        ("logit": -D's logit; "nsgan": -log D) + prior * mean(z^2), both networks as under model.eval().
        -> (z' [n,100], logit_before [n], logit_after [n]); logit_after is score_latents(z')."""
        if mode not in ("nsgan", "logit"):
            raise JckError(f"refine: mode must be 'nsgan' or 'logit', got {mode!r}")
        z = z.reshape(-1, 100)
        before = self.score_latents(z, labels)[0]
        z2, _ = self.project(None, labels, steps=steps, lr=lr, prior=prior, z0=z, critic=mode, critic_weight=1.0)
        return z2, before, self.score_latents(z2, labels)[0]

    def _score_ready(self, what):
        if not self._shared.get("d_loaded"):
            raise JckError(f"{what}: this engine's discriminator was never loaded or trained (load_state with a model_d state, "
                           f"Sampler.from_checkpoint(..., with_d=True)); it would score with all-zero weights")
        self._current()

    def _score_labels(self, what, labels, n):
        if self.family != 1:
            return None
        if labels is None or tuple(labels.shape) != (n, 100):
            raise JckError(f"CGAN {what} needs one-hot int64 labels [n,100]")
        return labels.to(self.device, torch.int64).contiguous()

    def _score_chunks(self, n, lab, zc=None, res=None, x=None, nz=None):
        """(logit [n], prob [n]) in chunks of at most `batch` rows: the eval-mode generator on zc's rows if given (their images to
        res, if given), then the discriminator on x's rows (+ the instance noise nz) or, x None, on the images where the generator
        left them"""
        logit = torch.empty(n, dtype=torch.float32, device=self.device)
        prob = torch.empty(n, dtype=torch.float32, device=self.device)
        for lo, hi in chunk_plan(n, self.batch):
            if zc is not None:
                self._sample_chunk(zc, lab, lo, hi, SAMPLE_EVAL, res)
            lib.jck_engine_score(self._h, _rows(x, lo, hi), _rows(nz, lo, hi), _rows(lab, lo, hi), hi - lo, logit[lo:hi], prob[lo:hi], cur_stream())
        return logit, prob

    def score(self, images, labels=None, noise=None):
        """(logit [n], prob [n]) fp32 on the device: the discriminator as under model.eval() - BatchNorm on its running statistics,
        Dropout the identity - so every image is scored on its own and nothing of the training state is written.
        images: fp32 NCHW [n,3,S,S] in [-1, 1], or uint8 NHWC [n,S,S,3] (taken as u8 / 127.5 - 1, hipgan.sampler.images_to_target);
        noise: None, or a tensor shaped like the fp32 images - D then sees 0.9 * image + 0.1 * noise, the trainers' instance noise.
        Any n: rows go through in chunks of at most `batch`, each row's numbers those of a call with that row alone."""
        x = fit_images(images, self.size, "score")
        n = x.shape[0]
        lab = self._score_labels("score", labels, n)
        nz = None
        if noise is not None:
            if tuple(noise.shape) != tuple(x.shape):
                raise JckError(f"score: noise must be shaped like the images {tuple(x.shape)}, got {tuple(noise.shape)}")
            nz = noise.to(self.device, torch.float32).contiguous()
        self._score_ready("score")
        x = x.to(self.device, torch.float32).contiguous()
        self._keep_score = (x, nz, lab)
        return self._score_chunks(n, lab, x=x, nz=nz)

    def score_latents(self, z, labels=None):
        """(logit [n], prob [n]) of D(G(z)), both networks as under model.eval(): per chunk of at most `batch` rows the eval-mode
        generator (sample(bn="running")) leaves its images on the device and the discriminator scores them where they lie."""
        return self.sample_scored(z, labels, out=None, _what="score_latents")[1:]

    def sample_scored(self, z, labels=None, out="float", _what="sample_scored"):
        """(images, logit [n], prob [n]): sample(z, bn="running", out=out) and score_latents(z) from ONE generator pass per chunk."""
        if out not in ("float", "uint8") and _what == "sample_scored":
            raise JckError(f"sample_scored: out must be 'float' or 'uint8', got {out!r}")
        n, zc, lab = self._latents(_what, z, labels)
        self._score_ready(_what)
        res = None if out is None else self._image_out(n, out)
        self._keep_score = (zc, lab)
        return (res,) + self._score_chunks(n, lab, zc=zc, res=res)

    def score_current(self, n, labels=None):
        """(logit [n], prob [n]) of the n images the generator produced last (sample(...) just before), scored where they lie."""
        if not 1 <= n <= self.batch:
            raise JckError(f"score_current: n must be in [1, {self.batch}]")
        lab = self._score_labels("score_current", labels, n)
        self._score_ready("score_current")
        self._keep_score = (lab,)
        return self._score_chunks(n, lab)

    def _feature_args(self, what, grid, pool):
        """(grid, jck_grid_pool's mode, the feature dimension F) of a features call, validated on the host"""
        if pool not in POOL_MODES:
            raise JckError(f"{what}: pool must be 'max' or 'mean', got {pool!r}")
        return int(grid), POOL_MODES[pool], feature_layout(self.size, grid)[1]

    def _feature_chunks(self, n, grid, mode, F, x=None, zc=None, lab=None):
        """fp32 [n, F] in chunks of at most `batch` rows: the eval-mode generator on zc's rows if given, then the discriminator's
        pooled activations of x's rows or, x None, of the images where the generator left them"""
        out = torch.empty(n, F, dtype=torch.float32, device=self.device)
        for lo, hi in chunk_plan(n, self.batch):
            if zc is not None:
                self._sample_chunk(zc, lab, lo, hi, SAMPLE_EVAL, None)
            lib.jck_engine_features(self._h, _rows(x, lo, hi), hi - lo, grid, mode, out[lo:hi], F, cur_stream())
        return out

    def features(self, images, grid=4, pool="max"):
        """fp32 [n, F] on the device: the discriminator as a feature extractor (Radford et al. 2016, section 5.1).  D runs as under
        model.eval() (score()), and every conv stage's LeakyReLU output is pooled - pool="max" or "mean" - to a grid x grid raster,
        flattened cell-major, channel-minor and concatenated, stage 0 first: hipgan.probe.feature_layout(size, grid) names the blocks
        (F = 960 grid^2 at 64 x 64).  images: fp32 NCHW [n,3,S,S] in [-1, 1] or uint8 NHWC [n,S,S,3].  No labels: a CGAN's conv stack
        never sees them.  Any n, rows independent bit for bit; nothing of the training state is written."""
        grid, mode, F = self._feature_args("features", grid, pool)
        x = fit_images(images, self.size, "features")
        self._score_ready("features")
        x = x.to(self.device, torch.float32).contiguous()
        self._keep_score = (x,)
        return self._feature_chunks(x.shape[0], grid, mode, F, x=x)

    def features_latents(self, z, labels=None, grid=4, pool="max"):
        """features() of G(z), both networks as under model.eval(): per chunk the eval-mode generator (sample(bn="running")) leaves
        its images on the device and the discriminator reads them where they lie.  labels: the generator's, CGAN only."""
        grid, mode, F = self._feature_args("features_latents", grid, pool)
        n, zc, lab = self._latents("features_latents", z, labels)
        self._score_ready("features_latents")
        self._keep_score = (zc, lab)
        return self._feature_chunks(n, grid, mode, F, zc=zc, lab=lab)
