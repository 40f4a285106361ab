"""DCGAN trainer for MI355X - drop-in for the reference's train/dcgan_trainer.py.

Same constructor `DCGANTrainer(args, model_g, model_d, data_pre)`, same `train()`, `save_model(typ, iters, value, images)`,
`compute_gradient_penalty(real, fake)`, same log line, same checkpoint dict {'model_g','model_d','optimizer_g','optimizer_d'}
and file names.  What differs is the execution: one iteration (reference train/dcgan_trainer.py:155-189) is a single native
schedule of gfx950 kernels (hipgan.engine.DcganEngine -> jck_engine_phase): the modules' parameters live in the engine's flat
arenas (zero copy), the six logged scalars stay on the device and are read back only when a line is logged, the optimiser
step is a fused flat Adam, and with torch.distributed initialised the D/G gradient arenas are all-reduced over RCCL (D's
reduction overlapping the gradient-penalty pass).  No CPU fallback.  The loop itself is train/gan_trainer.py's, shared with CGAN.
"""
import argparse
import os
from datetime import datetime

import torch
import torch.nn as nn

from hipgan.engine import DcganEngine
from model.DCGAN import weights_init
from train.gan_trainer import (EVAL_EVERY, HIGHER, LOG_EVERY, LOWER, GANTrainer, _make_grid, _save_png,  # noqa: F401 (re-exported)
                               inception_input, score_on_device)


class DCGANTrainer(GANTrainer):
    ENGINE, WEIGHTS_INIT, ANNOUNCE_NEXT = DcganEngine, staticmethod(weights_init), True
    CRITERIA = (("fid", LOWER, 1e10, "fid", "lowest fid"), ("is", HIGHER, 0, "is", "highest is"), ("kid", LOWER, 1e10, "kid", "lowest kid"))

    def __init__(self, args: argparse.Namespace, model_g: nn.Module, model_d: nn.Module, data_pre, prec=None, host_rng=None,
                 gp_backward=None):
        """prec, host_rng: as GANTrainer.
        gp_backward (default: args.gp_backward, 0): 1 back-propagates the gradient penalty into D (error_d = error_real + error_fake
        + 10 * gp is what D descends on); 0 is the reference, which computes error_d but never calls backward on it (:178-179)."""
        self.gp_backward = bool(int(getattr(args, "gp_backward", 0) if gp_backward is None else gp_backward))
        super().__init__(args, model_g, model_d, data_pre, prec, host_rng)

    def _engine_kwargs(self, args):
        return {"image_size": getattr(self.model_g, "image_size", 64),     # 128: the configs[4] topology
                "gp_backward": self.gp_backward}                           # the tail-batch engines share it

    def _save_dir(self, args):
        datetime_now = args.model_path if getattr(args, "model_path", "") != "" else datetime.now().strftime("%Y%m%d_%H%M%S")
        return os.path.join(".", "save", "dcgan", datetime_now)

    # ------------------------------------------------------------------------------------------------------
    def save_model(self, typ, iters, value, images, snapshot=None):
        """snapshot: the state captured at the evaluation iteration (train/async_eval.py); None = the live state."""
        save_path = self._write_checkpoint(typ, f"{iters}_{value:.04f}", snapshot)
        if save_path is None:
            return
        _save_png(os.path.join(save_path, f"{iters}_fake_image.png"), _make_grid(images, padding=2, normalize=True), "fake images")
        self.logger.debug(f"{iters} model save")

    def _save_best(self, typ, iters, scores, images, snap):
        self.save_model(typ, iters, scores.get(typ, 0.0), images, snap)     # the folder is named after its score; `latest` has none

    def compute_gradient_penalty(self, real_data, fake_data):
        """Stand-alone value of the penalty (reference :110-127) through the autograd Functions of the HIP path."""
        alpha = torch.rand(real_data.size(0), 1, 1, 1, device=self.device)
        inter = (alpha * real_data + ((1 - alpha) * fake_data)).detach().requires_grad_(True)
        d_inter = self.model_d(inter)
        grads = torch.autograd.grad(outputs=d_inter, inputs=inter, grad_outputs=torch.ones_like(d_inter))[0]
        grads = grads.view(grads.size(0), -1)
        return ((grads.norm(2, dim=1) - 1) ** 2).mean()

    # ------------------------------------------------------------------------------------------------------
    def _evaluate(self, fixed_noise, iters, best):
        """Device part of the evaluation (reference :198-212) on a side stream; training resumes behind the sampling kernels
        only (train/async_eval.py).  The host part runs in _finish_eval."""
        self._finish_eval(best, wait=True)          # the evaluation of 500 iterations ago, if its host part is still owed
        eng = self._sampler_for(fixed_noise.size(0))

        def device_part(fake):
            if self.metric is None:
                return {"images": fake}
            x = inception_input(fake)                # :202-206 in one device pass
            return {"images": x, **score_on_device(self.metric, self.extra_metrics, x, intra=False)}
        self._eval.launch(iters, lambda: eng.sample(fixed_noise), device_part)      # sample: one train-mode BN batch (:199-200)

    # ---- the draws of a run and of a step ------------------------------------------------------------------
    def _fixed_inputs(self):
        noise = torch.randn(64, 100, 1, 1).to(self.device) if self.host_rng else torch.randn(64, 100, 1, 1, device=self.device)
        return (noise,), ()

    def _host_noise(self, b, labels):
        hg = self.host_gen              # reference order: train/dcgan_trainer.py:160,168,171,111
        return {"n1": torch.randn(b, 3, 64, 64, generator=hg), "z": torch.randn(b, 100, 1, 1, generator=hg),
                "n2": torch.randn(b, 3, 64, 64, generator=hg), "alpha": torch.rand(b, 1, 1, 1, generator=hg)}

    def _device_noise(self, eng, labels):
        """None: the step draws inside its own kernels - unless the rank has a noise stream of its own (data parallel)."""
        return eng.draw_noise(self.noise_gen, fast=eng.fast_noise) if self.noise_gen is not None else None
