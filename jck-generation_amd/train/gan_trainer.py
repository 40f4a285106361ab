"""What the DCGAN and the CGAN trainer share: construction around a native step engine, the training loop, the deferred
evaluation's best-score ladder, checkpoints.  train/dcgan_trainer.py and train/cgan_trainer.py hold what differs between the
families (the drop-in signatures, the draws of a step, the evaluation's device part, the pictures)."""
import operator
import os
import struct
import time
import zlib

import numpy as np
import torch
import torch.nn as nn

from hipgan.dist import GradReducer, ReplicaGuard
from hipgan.engine import SCALAR_NAMES, DeviceBatch
from hipgan.optim import EngineAdam
from logger.main_logger import MainLogger
from logger.utils import time_to_str
from train.async_eval import AsyncEval, snapshot_to_cpu
from train.trainer import Trainer
from utils import require_gpu

EVAL_EVERY, LOG_EVERY = 500, 100          # train/dcgan_trainer.py:198,191


def inception_input(fake):
    """[-1,1] images [N,3,64,64] on the device -> what the metric network is fed (reference :202-206): 0.5*x + 0.5,
    F.resize to 299x299 (bilinear), ImageNet normalisation - fused in jck_resize_norm."""
    from hipgan import lib
    from hipgan._lib import cur_stream
    fake = fake.to(torch.float32).contiguous()
    n = fake.size(0)
    out = torch.empty(n, 3, 299, 299, dtype=torch.float32, device=fake.device)
    mean = torch.tensor([0.485, 0.456, 0.406], device=fake.device)
    std = torch.tensor([0.229, 0.224, 0.225], device=fake.device)
    lib.jck_resize_norm(fake, out, n, 3, fake.size(2), fake.size(3), 299, 299, 0.5, 0.5, mean, std, cur_stream())
    return out


def score_on_device(metric, extra_metrics, x, intra):
    """Device part of the scores of one evaluation: ONE pass of the metric network over the 299x299 images x (IS and FID are
    scored on the same features), then the fp64 mean / covariance of the logits on the device (all of them, and per superclass
    with intra) and, with --extra_metrics, the KID sums and manifold hits (csrc/pairstat.hip)."""
    logits = metric.logits(x)
    out = {"logits": logits}
    if logits.is_cuda:
        out.update(metric.fake_stats_device(logits, intra=intra))
        if extra_metrics:
            out.update(metric.fake_pair_stats_device(logits, intra=intra))
    return out


def _as_tensor(batch):
    """fp32 NCHW view of a loader batch (a DeviceBatch is transformed on the device first)."""
    return batch.materialize() if isinstance(batch, DeviceBatch) else batch


def _make_grid(images, nrow=8, padding=2, normalize=True):
    """Minimal stand-in for torchvision.utils.make_grid (absent in this image): [N,3,H,W] -> [3,H',W']."""
    x = images.detach().float().cpu()
    if normalize:
        lo, hi = float(x.min()), float(x.max())
        x = (x - lo) / max(hi - lo, 1e-5)
    n, c, h, w = x.shape
    ncol = min(nrow, n)
    nr = (n + ncol - 1) // ncol
    grid = torch.zeros(c, nr * (h + padding) + padding, ncol * (w + padding) + padding)
    for i in range(n):
        r, q = divmod(i, ncol)
        grid[:, padding + r * (h + padding):padding + r * (h + padding) + h,
             padding + q * (w + padding):padding + q * (w + padding) + w] = x[i]
    return grid


def _encode_png(hwc_u8):
    """uint8 [H,W,3] (or [H,W]: grey) -> the bytes of an 8-bit PNG, with zlib and struct alone (no matplotlib, no Pillow): one
    IDAT, filter type 0 on every row.  For the generate CLI; the trainers keep _save_png."""
    a = np.ascontiguousarray(np.asarray(hwc_u8))
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError(f"_encode_png wants uint8 [H,W,3] or [H,W], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, -1)], axis=1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b"")


def _save_png(path, chw, title=None):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        plt.clf()
        plt.axis("off")
        if title:
            plt.title(title)
        plt.imshow(np.transpose(chw.numpy(), (1, 2, 0)))
        plt.savefig(path)
        plt.close("all")
    except Exception as e:          # plotting is cosmetic; never take the run down
        MainLogger().warning(f"could not write {path}: {e}")


LOWER, HIGHER = operator.lt, operator.gt


class GANTrainer(Trainer):
    """A family sets
      ENGINE, WEIGHTS_INIT    its step engine (hipgan.engine) and its model file's weights_init
      ANNOUNCE_NEXT           whether a step is told the next real batch (step_async next_real; PHASE_D_REAL_FWD is DCGAN's)
      INTRA, EVAL_IMAGES      whether evaluation scores per superclass too; the key of the evaluation's pictures in its host dict
      CRITERIA                the best-score ladder, tested and saved in this order: (score key, LOWER / HIGHER is better,
                              initial best, checkpoint folder, log word); a criterion whose score is absent is passed over
    and defines _save_dir, _fixed_inputs, _host_noise, _device_noise, _evaluate, _save_best, save_model, and where it differs
    from the defaults here _engine_kwargs, _unpack, _after_eval."""
    ENGINE = WEIGHTS_INIT = None
    ANNOUNCE_NEXT = INTRA = False
    EVAL_IMAGES = "images"
    CRITERIA = ()

    def __init__(self, args, model_g, model_d, data_pre, prec=None, host_rng=None, **engine_kw):
        """prec: "bf16" (fast, default), "f32" (exact-fp32 parity path) or "bf16x3" (fp32 storage, split-bf16 GEMMs: tracks
        the reference within 1e-3 per step at several times the f32 path's speed); env JCKGAN_PREC.
        host_rng: draw every random tensor from the CPU generator in the reference's order and upload it (bit-identical
        noise to a CPU run of the reference; env JCKGAN_HOST_RNG=1).  Default: Philox on the device.
        engine_kw: further arguments of the engine's constructor, after the family's own (_engine_kwargs)."""
        self.logger = MainLogger(args)
        self.device = require_gpu(type(self).__name__)
        self.epoch = args.epoch
        self.max_lr = args.max_learning_rate
        self.lambda_gp = 10.0
        self.extra_metrics = bool(int(getattr(args, "extra_metrics", 0)))      # --extra_metrics 1: KID, precision / recall beside IS / FID
        self.prec = prec or os.environ.get("JCKGAN_PREC", "bf16")

        self.host_rng = bool(int(os.environ.get("JCKGAN_HOST_RNG", "0"))) if host_rng is None else host_rng
        if self.host_rng:       # weights_init must consume the CPU generator, as it does in a CPU run of the reference
            model_g.apply(self.WEIGHTS_INIT)
            model_d.apply(self.WEIGHTS_INIT)
        self.model_g = model_g.to(self.device)
        self.model_d = model_d.to(self.device)
        n_g = sum(p.numel() for p in self.model_g.parameters())
        n_d = sum(p.numel() for p in self.model_d.parameters())
        self.logger.debug(f"Generator: {n_g} parameters\n{self.model_g}")
        self.logger.debug(f"Discriminator: {n_d} parameters\n{self.model_d}")
        if not self.host_rng:   # reference order (train/dcgan_trainer.py:46-55): move, then initialise on the device
            self.model_g.apply(self.WEIGHTS_INIT)
            self.model_d.apply(self.WEIGHTS_INIT)
        self.model_g.prec = self.model_d.prec = self.prec

        self.data_pre = data_pre
        self.train_loader, metric_loader = self.data_pre.get_data_loader()
        self.metric = self._make_metrics(metric_loader)

        # data parallel: identical initial weights on every rank, gradients all-reduced per step
        self.world, self.rank = 1, 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world, self.rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
        self.batch_size = int(getattr(args, "batch_size", 128))
        self.engine = self.ENGINE(batch=self.batch_size, prec=self.prec, device=self.device, **self._engine_kwargs(args), **engine_kw,
                                  ema_decay=getattr(args, "ema_decay", None), ema_start=int(getattr(args, "ema_start", 0)))
        self.engine.adopt_modules(self.model_g, self.model_d)
        if self.world > 1:
            for key in ("g_params", "d_params", "g_bn", "d_bn"):
                torch.distributed.broadcast(self.engine.arenas[key], src=0)
            self.engine.mark_weights_changed()
        self._tail_engines, self._ema_samplers = {}, {}
        self.reducer = GradReducer(self.world) if self.world > 1 else None
        # every rank must hold the same parameters after a step: checked after the first steps and at every evaluation point; on a
        # mismatch the state is re-broadcast and the engines fall back to the plain all-reduce schedule (hipgan/dist.py)
        self.guard = (ReplicaGuard(lambda: [self.engine] + list(self._tail_engines.values()), self.world, log=self.logger.debug)
                      if self.world > 1 else None)
        # data parallel: main.py seeds every rank alike (identical initial weights), so the NOISE needs its own per-rank stream -
        # otherwise every replica draws the same z / instance noise / alpha, generates the same fake batch, and the all-reduce
        # averages N identical gradients (effective batch B instead of N*B for G and for the fake half of D)
        self.noise_gen = self.host_gen = None
        if self.world > 1:
            from change_randomseed import RANDOMSEED
            self.noise_gen = torch.Generator(device=self.device).manual_seed(RANDOMSEED + 1 + self.rank)
            self.host_gen = torch.Generator().manual_seed(RANDOMSEED + 1 + self.rank)
        # The step's own draws (z, alpha, instance noise, CGAN's dropout masks: Philox keyed by this seed and the step) follow the
        # run's seed on ONE GPU too: in the reference change_randomseed.RANDOMSEED / torch.manual_seed govern all of it
        # (main.py:31-37), so a different seed must give a different noise sequence here as well.
        from change_randomseed import RANDOMSEED as _SEED
        self._noise_seed = (int(torch.initial_seed()) ^ (_SEED << 20)) + 1 + self.rank
        self.engine.set_noise_seed(self._noise_seed)

        self.optimizer_g = EngineAdam(self.engine, "g", self.model_g.named_parameters(), self.max_lr, betas=[0.5, 0.999])
        self.optimizer_d = EngineAdam(self.engine, "d", self.model_d.named_parameters(), self.max_lr, betas=[0.5, 0.999])
        self.criterion = nn.BCELoss()       # kept for API parity; the step uses the fused head kernel (same -100 clamp)

        self.model_save_path = self._save_dir(args)
        os.makedirs(self.model_save_path, exist_ok=True)
        self.logger.debug(f"save path: {self.model_save_path}")

    def _engine_kwargs(self, args):
        return {}

    # ------------------------------------------------------------------------------------------------------
    def _make_metrics(self, metric_loader):
        try:
            from metrics import Metrics
            # --data: the cache of the real features is named after that file (preprocess/dcgan_data_preprocessor.py), never the
            # default ./data/metric_data.pikl, which holds CIFAR-100's and would be reused silently
            cache = getattr(self.data_pre, "metric_cache", None)
            return Metrics(metric_loader, cache=cache) if cache else Metrics(metric_loader)
        except Exception as e:
            self.logger.warning(f"Inception-score / FID evaluation disabled: {e}")
            return None

    def _engine_for(self, b):
        if b == self.batch_size:
            return self.engine
        if b not in self._tail_engines:
            self._tail_engines[b] = type(self.engine)(batch=b, share=self.engine)
            self._tail_engines[b].set_noise_seed(self._noise_seed)
        return self._tail_engines[b]

    def _sampler_for(self, n):
        """The engine evaluation samples n images from: the averaged generator when the engine keeps one (--ema_decay; its own
        BatchNorm running statistics, the live generator's stay where training left them), else the live one as the reference does."""
        if self.engine.ema_decay is None:
            return self._engine_for(n)
        if n not in self._ema_samplers:
            self._ema_samplers[n] = type(self.engine)(batch=n, share=self.engine, ema=True)
        return self._ema_samplers[n]

    # ------------------------------------------------------------------------------------------------------
    def _write_checkpoint(self, typ, file_stem, snapshot):
        """<save dir>/<typ>/<file_stem>.pt in place of the folder's older checkpoints, on rank 0 -> the folder (None elsewhere).
        snapshot: the state captured at the evaluation iteration (train/async_eval.py); None = the live state."""
        if self.rank != 0:
            return None
        self.engine.join()                      # the G phase of the last step may still be in flight on its stream
        save_path = os.path.join(self.model_save_path, typ)
        os.makedirs(save_path, exist_ok=True)
        for filename in os.listdir(save_path):
            fp = os.path.join(save_path, filename)
            if os.path.isfile(fp) and filename.endswith(".pt"):
                os.remove(fp)
        state = snapshot_to_cpu(snapshot) if snapshot is not None else {
            "model_g": {k: v.detach().cpu().clone() for k, v in self.model_g.state_dict().items()},
            "model_d": {k: v.detach().cpu().clone() for k, v in self.model_d.state_dict().items()},
            "optimizer_g": self.optimizer_g.state_dict(), "optimizer_d": self.optimizer_d.state_dict()}
        if snapshot is None and self.engine.ema_decay is not None:
            state["model_g_ema"] = self.engine.ema_state_dict()
        self.engine.check()                     # (the copies above synchronised) never checkpoint a step whose grid barrier timed out
        torch.save(state, os.path.join(save_path, f"{file_stem}.pt"))
        return save_path

    def load_model(self, path):
        """Resume from a checkpoint written by save_model() or by the reference (its load_model is commented out)."""
        saved = torch.load(path, map_location="cpu", weights_only=False)
        self.model_g.load_state_dict(saved["model_g"])
        self.model_d.load_state_dict(saved["model_d"])
        self.optimizer_g.load_state_dict(saved["optimizer_g"])
        self.optimizer_d.load_state_dict(saved["optimizer_d"])
        if self.engine.ema_decay is not None:       # a checkpoint written without --ema_decay: the average starts at its weights
            if "model_g_ema" in saved:
                self.engine.load_ema_state(saved["model_g_ema"])
            else:
                self.engine.reset_ema()
        self.engine.mark_weights_changed()

    # ------------------------------------------------------------------------------------------------------
    def _finish_eval(self, best, wait):
        """Host part of a launched evaluation (_evaluate), once its device part has finished: scores, log lines, a checkpoint
        for every criterion that improved - or `latest` when there is no metric network."""
        p = self._eval.take(wait)
        if p is None:
            return
        iters, host, snap = p["iters"], p["host"], p["snapshot"]
        images = host[self.EVAL_IMAGES]
        if "logits" in host:
            if "mu" in host:
                vals = self.metric.scores_from_stats(host["logits"], host, intra=self.INTRA)
            else:
                vals = self.metric.scores_from_logits(host["logits"], intra=self.INTRA)
            scores = dict(zip(("is", "fid", "intra"), vals))
            self.logger.debug(f"inception score: {scores['is']}\tfid: {scores['fid']}"
                              + (f"\tintra fid: {scores['intra']}" if self.INTRA else ""))
            if "kid_rr" in host:
                extra = self.metric.extra_scores_from_stats(host, intra=self.INTRA)
                self.logger.debug(f"kid: {extra['kid']}\tprecision: {extra['precision']}\trecall: {extra['recall']}"
                                  + (f"\tintra kid: {extra['intra_kid']}" if self.INTRA else ""))
                scores.update(extra)
            for key, better, initial, folder, word in self.CRITERIA:
                if key in scores and better(scores[key], best.setdefault(key, initial)):
                    best[key] = scores[key]
                    self.logger.debug(f"{iters} {word}")
                    self._save_best(folder, iters, scores, images, snap)
        else:
            self._save_best("latest", iters, {}, images, snap)
        self._after_eval(iters, images)

    def _after_eval(self, iters, images):
        pass

    # ------------------------------------------------------------------------------------------------------
    def _unpack(self, data):
        """loader item -> (real batch on the device, labels on the device or None)"""
        real = data[0] if isinstance(data[0], DeviceBatch) else data[0].to(self.device, torch.float32, non_blocking=True).contiguous()
        return real, None

    def train(self):
        loader = self.train_loader
        n_iter = self.epoch * len(loader)
        fixed, eval_dirs = self._fixed_inputs()
        best = {}
        self._eval = AsyncEval(self)
        if self.rank == 0:
            real_batch = next(iter(loader))
            _save_png(os.path.join(self.model_save_path, "real_image.png"),
                      _make_grid(_as_tensor(real_batch[0])[:64], padding=5, normalize=True), "real images")
        history = torch.zeros(max(n_iter, 1), len(SCALAR_NAMES), device=self.device)     # every step's scalars, on the device
        reduce = self.reducer.start if self.reducer else None
        look_ahead = self.ANNOUNCE_NEXT and not self.host_rng
        start = time.time()
        self.logger.debug("train start")
        iters = 0
        for epoch in range(self.epoch):
            if hasattr(getattr(loader, "sampler", None), "set_epoch"):
                loader.sampler.set_epoch(epoch)                   # host-data path: a new shuffle / shard every epoch
            it, nxt_dev = iter(loader), None
            nxt = next(it, None)
            for i in range(len(loader)):
                if nxt is None:
                    break
                real, labels = nxt_dev if nxt_dev is not None else self._unpack(nxt)
                nxt = next(it, None)
                # the next batch is announced to the step, which runs the forward half of its D(real) pass under G's gradient
                # all-reduce (data parallel) / beside Adam(G) and the repack (one GPU): hipgan/engine.py step_async next_real;
                # same-sized batches only (one engine per size)
                nxt_dev = self._unpack(nxt) if (look_ahead and nxt is not None) else None
                same_size = nxt_dev is not None and nxt_dev[0].size(0) == real.size(0)
                announce = {"next_real": nxt_dev[0] if same_size else None} if self.ANNOUNCE_NEXT else {}
                eng = self._engine_for(real.size(0))
                noise = self._host_noise(real.size(0), labels) if self.host_rng else self._device_noise(eng, labels)
                eng.step_async(real, noise, self.optimizer_d.lr, reduce_d=reduce, reduce_g=reduce, grad_scale=1.0 / self.world,
                               **announce)
                eng.record_scalars(history[iters])
                if i % LOG_EVERY == 0:
                    self._finish_eval(best, wait=False)              # host part of a finished evaluation (scores, checkpoint)
                    s = eng.scalars()                                # the only host sync of the iteration
                    self.logger.debug(f"[{epoch}/{self.epoch}][{i}/{len(loader)}]\tloss_d: {s['loss_d']:.4f}\tloss_g: {s['loss_g']:.4f}"
                                      + f"\tD(x): {s['d_x']:.4f}\tD(G(z)): {s['d_gz1']:.4f} / {s['d_gz2']:.4f}")
                at_eval = (iters % EVAL_EVERY == 0) or ((epoch == self.epoch - 1) and (i == len(loader) - 1))
                if self.guard is not None and (iters == 2 or (at_eval and iters > 2)):
                    self.guard.check(f"after iteration {iters} ")
                if at_eval:
                    self._evaluate(*fixed, iters, best, *eval_dirs)
                iters += 1
        self._finish_eval(best, wait=True)
        self.engine.join()
        torch.cuda.synchronize()
        self.engine.check()
        end = time.time()
        self.logger.debug(f"train finish\ttiem: {time_to_str(end - start)}")
        hist = history[:iters].cpu()
        self.losses_d, self.losses_g = hist[:, 0].tolist(), hist[:, 1].tolist()
        if self.rank == 0:
            self._plot_losses()
        return self.losses_d, self.losses_g

    def _plot_losses(self):
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            plt.clf()
            plt.figure(figsize=(8, 6))
            x = range(1, len(self.losses_g) + 1)
            plt.plot(x, self.losses_d, label="Discriminator Loss")
            plt.plot(x, self.losses_g, label="Generator Loss")
            plt.title("Discriminator and Generator Loss")
            plt.xlabel("Iterations")
            plt.ylabel("Loss")
            plt.legend()
            plt.savefig(os.path.join(self.model_save_path, "loss.png"))
            plt.close("all")
        except Exception as e:
            self.logger.warning(f"could not write loss.png: {e}")
