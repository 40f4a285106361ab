"""CGAN trainer for MI355X - drop-in for the reference's train/cgan_trainer.py: `CGANTrainer(args, model_g, model_d, data_pre)`,
`train()`, `save_model(typ, iters, inception_score, fid, intra_fid, images)`, `save_image(path, iters, images)`,
`compute_gradient_penalty(real, fake, labels)`; same log line and checkpoint dict.  One iteration (reference :173-213) is the
native engine schedule of family 1: D(real), G(z,l), D(fake), the gradient penalty INCLUDING its back-propagation (double
backward, closed form), Adam(D), D(fake) again, backward into G, Adam(G).  The loop itself is train/gan_trainer.py's, shared
with DCGAN."""
import os

import numpy as np
import torch

from hipgan.engine import CganEngine
from model.CGAN import weights_init
from train.gan_trainer import HIGHER, LOWER, GANTrainer, inception_input, score_on_device


class CGANTrainer(GANTrainer):
    ENGINE, WEIGHTS_INIT, INTRA, EVAL_IMAGES = CganEngine, staticmethod(weights_init), True, "denorm"
    CRITERIA = (("fid", LOWER, 1e10, "fid", "lowest fid"), ("intra", LOWER, 1e10, "intra_fid", "lowest intra fid"),
                ("is", HIGHER, 0, "is", "highest is"), ("kid", LOWER, 1e10, "kid", "lowest kid"),
                ("intra_kid", LOWER, 1e10, "intra_kid", "lowest intra kid"))

    def __init__(self, args, model_g, model_d, data_pre, prec=None, host_rng=None):
        """prec: "bf16" (default), "f32" or "bf16x3"; env JCKGAN_PREC.  host_rng: the CPU generator's noise; as GANTrainer."""
        super().__init__(args, model_g, model_d, data_pre, prec, host_rng)

    def _save_dir(self, args):
        return args.save_path                       # reference :66

    # ------------------------------------------------------------------------------------------------------
    def save_model(self, typ, iters, inception_score, fid, intra_fid, images, snapshot=None):
        save_path = self._write_checkpoint(typ, f"{iters}_{inception_score:.04f}_{fid:.04f}_{intra_fid:.04f}", snapshot)
        if save_path is not None:
            self.save_image(save_path, iters, images)

    def _save_best(self, typ, iters, scores, images, snap):
        self.save_model(typ, iters, scores.get("is", 0.0), scores.get("fid", 0.0), scores.get("intra", 0.0), images, snap)

    def save_image(self, path, iters, images):
        """10x10 grid, one image per class, titled with the class name (reference :93-103)."""
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            plt.clf()
            fig = plt.figure(figsize=(10, 10))
            for i in range(min(100, images.shape[0])):
                fig.add_subplot(10, 10, i + 1)
                plt.title(self.data_pre.idx_to_labels[i])
                plt.axis("off")
                plt.imshow(np.clip(np.transpose(images[i].numpy(), (1, 2, 0)), 0, 1))
            plt.savefig(os.path.join(path, f"{iters}_fake_image.png"))
            plt.close("all")
        except Exception as e:
            self.logger.warning(f"could not write the class grid: {e}")

    def compute_gradient_penalty(self, real_data, fake_data, labels_data):
        """The reference's penalty (:114-131) as a tensor that can be back-propagated into D's parameters, as :200-203 do
        (`error_d = error_real + error_fake + 10 * gp; error_d.backward()`): hipgan.functional.gradient_penalty, whose backward
        is the engine's closed-form double backward.  train() itself runs the penalty inside the native step."""
        from hipgan import functional as HF
        return HF.gradient_penalty(self.model_d, real_data.detach(), fake_data.detach(), labels=labels_data)

    # ------------------------------------------------------------------------------------------------------
    def _evaluate(self, fixed_noise, fixed_labels, iters, best, image_save_path):
        """Device part of the evaluation (reference :222-252) on a side stream (train/async_eval.py): 1000 images = ONE
        BatchNorm batch as in the reference, the fused 299x299 resize + normalise, ONE pass of the metric network, fp64 mean /
        covariance of the logits (all 1000 and per superclass) - training resumes behind the sampling kernels only."""
        self._finish_eval(best, wait=True)
        eng = self._sampler_for(fixed_noise.size(0))
        self._image_save_path = image_save_path

        def device_part(fake):
            out = {"denorm": (0.5 * fake + 0.5)[::10].contiguous()}
            if self.metric is not None:     # :227-231 in one device pass, then the metric network
                out.update(score_on_device(self.metric, self.extra_metrics, inception_input(fake), intra=True))
            return out
        self._eval.launch(iters, lambda: eng.sample(fixed_noise, fixed_labels), device_part)

    def _after_eval(self, iters, images):
        if self.rank == 0:
            self.save_image(self._image_save_path, iters, images)

    # ---- the draws of a run and of a step ------------------------------------------------------------------
    def _fixed_inputs(self):
        dev = self.device
        # 100 classes x 10 samples (reference :144-153); the draw order matters in host-RNG mode
        noises = [torch.randn(10, 100, 1, 1) if self.host_rng else torch.randn(10, 100, 1, 1, device=dev) for _ in range(100)]
        labels = torch.nn.functional.one_hot(torch.arange(100).repeat_interleave(10), 100).to(torch.int64).to(dev)
        image_save_path = os.path.join(self.model_save_path, "img")
        os.makedirs(image_save_path, exist_ok=True)
        return (torch.vstack(noises).to(dev), labels), (image_save_path,)

    def _unpack(self, data):
        return super()._unpack(data)[0], data[1].to(self.device, torch.int64, non_blocking=True).contiguous()

    def _host_noise(self, b, labels):
        hg = self.host_gen              # CPU generator in the reference's order (:181,183[dropout],189,192,194,115,118,209)
        keep = lambda: torch.empty(b, 256).bernoulli_(0.75, generator=hg)
        noise = {"n1": torch.randn(b, 3, 64, 64, generator=hg)}
        noise["m1"] = keep()
        noise["z"] = torch.randn(b, 100, 1, 1, generator=hg)
        noise["n2"] = torch.randn(b, 3, 64, 64, generator=hg)
        noise["m2"] = keep()
        noise["alpha"] = torch.rand(b, 1, 1, 1, generator=hg)
        noise["m3"] = keep()
        noise["m4"] = keep()
        noise["labels"] = labels
        return noise

    def _device_noise(self, eng, labels):
        return eng.draw_noise(self.noise_gen, labels=labels, fast=eng.fast_noise)
