"""Images from a trained generator, outside the trainer.  Run from this directory:

    python generate.py -m DCGAN --checkpoint ../model/DCGAN/fid/best.pt --num 64 --out samples
    python generate.py -m CGAN --checkpoint best.pt --num 8 --classes 3,17,42 --truncation 0.7 --out samples
    python generate.py -m DCGAN --checkpoint best.pt --interpolate 4:8 --which ema --calibrate 20 --out samples
    python generate.py -m DCGAN --checkpoint best.pt --project samples/images.npz --project_steps 300 --out projected
    python generate.py -m DCGAN --checkpoint best.pt --num 64 --select top --oversample 8 --score --out best_of
    python generate.py -m DCGAN --checkpoint best.pt --score_images samples/images.npz --out scored
    python generate.py -m DCGAN --checkpoint best.pt --num 64 --neighbours train.npz --k 4 --out samples
    python generate.py -m DCGAN --checkpoint best.pt --inpaint samples/images.npz --mask center:32 --out inpainted
    python generate.py -m DCGAN --checkpoint best.pt --num 64 --refine 10 --out refined
    python generate.py -m DCGAN --checkpoint best.pt --features train.npz --out feats
    python generate.py -m DCGAN --checkpoint best.pt --probe train.npz --probe_test test.npz --k 5 --out probe
    python generate.py -m DCGAN --checkpoint best.pt --num 64 --neighbours train.npz --space d --out samples
    python generate.py -m DCGAN --checkpoint best.pt --project samples/images.npz --project_feature_weight 10 --out perceptual
    python generate.py -m DCGAN --checkpoint best.pt --anomaly queries.npz --anomaly_lam 0.1 --out anomaly

Writes <out>/images.npz (images: uint8 [N,S,S,3]; z: fp32 [N,100]; labels: int64 class ids [N], CGAN only) and <out>/grid.png.
BatchNorm runs on the running statistics by default (--bn running): every image is a function of its own z, and --num is not
bounded by the batch.  --bn batch is the trainers' evaluation sampling: each chunk of -b images is one train-mode BatchNorm batch.
An averaged generator (--which ema, or auto when the file has one) wants --calibrate K first: K train-mode batches that fit the
running statistics to the averaged weights (in this process only; the file is not touched).
--project FILE.npz fits a latent to every picture of the file's `images` array (uint8 [n,S,S,3]: an images.npz of this tool, or any
such array; a CGAN takes the file's `labels` or cycles through --classes) by Adam through the frozen eval-mode generator and writes
<out>/projected.npz (z: fp32 [n,100]; loss: the mean squared error of each reconstruction in [-1, 1] units; images: the
reconstructions, uint8) and <out>/projected.png, each row of targets above the row of their reconstructions.
The checkpoint's discriminator (`model_d`), as under Discriminator.eval(): --score adds `logit` and `prob` fp32 [N] to images.npz;
--select top|drs with --oversample M keeps the --num best of M * --num draws, or runs discriminator rejection sampling with rounds
of that size (Sampler.images; a CGAN ranks within one class: --classes ID, else one drawn from the seed); --score_images FILE.npz scores an existing uint8 `images` array into <out>/scores.npz (logit, prob).
Whether the discriminator's running statistics make it a good ranker is a property of the run that trained it.
--neighbours REF.npz (with a sampling run, or with --score_images, whose images it then takes) looks up the --k nearest images of
REF's uint8 `images` array (the samples' size, or 32x32 training data, upscaled as the trainers do) for every sample, in pixel space:
<out>/neighbours.npz (idx int64 [n,k]; d2 squared distance in [-1, 1] units; rmse = sqrt(d2 / D); ref_nn_d2: the nearest other
reference image's d2 from the image idx[:,0]; copy = d2[:,0] < ref_nn_d2) and <out>/neighbours.png, each sample followed by its neighbours.
--inpaint FILE.npz --mask SPEC is semantic inpainting (Yeh et al. 2017; Sampler.inpaint): SPEC names the KNOWN pixels of the file's
pictures ("center:K": a centred K x K hole; "half:left|right|top|bottom": that half is the hole; an .npz / .npy file holding `mask`),
z is fitted to them alone (--project_steps, --project_lr) with --critic_weight W times -log D(G(z)) as the realism prior (0: none, no
discriminator needed), and <out>/inpainted.npz holds z, loss, term, known, images (G(z)) and completed (the known pixels of the input,
the holes from G); <out>/inpainted.png has one row per picture: masked input, G(z), completed.
--refine STEPS (with a sampling run) moves every latent STEPS Adam updates (--refine_lr) along the discriminator's gradient before its
image is made; images.npz then holds the refined z and gains logit_before / logit_after.
The discriminator as a feature extractor (Radford et al. 2016, section 5.1; hipgan.probe): --features FILE.npz pools every conv stage's
activation of the file's pictures (the discriminator's size, or 32x32 data, upscaled as the trainers do) to a --feature_grid raster
(--feature_pool max|mean) and writes <out>/features.npz (features: fp32 [n,F], unnormalised; layout: int64 [stages,4] rows of stage,
col0, C, H; grid; pool; labels if the file has them) for an external classifier.  --probe TRAIN.npz --probe_test TEST.npz (both with
`labels`) classifies every test picture by the majority of its --k (default 5) nearest training pictures in block-normalised feature
space and writes <out>/probe.json (accuracy, per_class, k, train, test, F, grid, pool).  --neighbours REF.npz --space d looks the
samples' neighbours up in that feature space instead of pixel space: neighbours.npz then holds idx, d2, ref_nn_d2 and copy, no rmse.
--project_feature_weight W (with --project) adds W times the mean squared distance between the discriminator's deepest-stage activations
of G(z) and of the picture to the projection's objective (perceptual projection; needs `model_d`).
--anomaly FILE.npz scores the file's pictures after AnoGAN (Schlegl et al. 2017; Sampler.anomaly): each is projected (--project_steps,
--project_lr) with a residual term and a feature-matching term on the discriminator's stage --anomaly_stage (default: the deepest),
and score = (1 - lam) residual + lam feature at the z reached (--anomaly_lam, default 0.1) - mean squared forms, not the paper's L1
sums.  <out>/anomaly.npz holds z, residual, feature, score, generated (G(z), uint8) and order (indices by falling score);
<out>/anomaly.png has one row per picture: input, G(z), |input - G(z)|; <out>/anomaly.json (auroc, n, anomalous, lam, stage) is written
when the file carries a bool `anomalous` [n] array."""
import argparse
import os
import sys

import numpy as np
import torch


def get_arg_parse(argv=None):
    p = argparse.ArgumentParser(description="sample a trained DCGAN / CGAN generator")
    p.add_argument("-m", "--model", choices=["DCGAN", "CGAN"], default="DCGAN")
    p.add_argument("--checkpoint", required=True, help="a checkpoint written by the trainers (or the reference's)")
    p.add_argument("--num", type=int, default=None, help="images, per class with --classes (default 64; not with --interpolate)")
    p.add_argument("-b", "--batch_size", type=int, default=64, help="images per launch sequence")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--truncation", type=float, default=None, help="draw z from a normal truncated to [-T, T]")
    p.add_argument("--bn", choices=["running", "batch"], default="running")
    p.add_argument("--which", choices=["auto", "live", "ema"], default="auto")
    p.add_argument("--calibrate", type=int, default=0, metavar="K", help="train-mode sampling batches before sampling")
    p.add_argument("--classes", type=parse_classes, default=None, metavar="3,17,...", help="CGAN: one grid row of --num images per class")
    p.add_argument("--interpolate", type=parse_interpolate, default=None, metavar="PAIRS:STEPS",
                   help="PAIRS spherical interpolations of STEPS points each between random z (one grid row per pair)")
    p.add_argument("--project", default=None, metavar="FILE.npz", help="fit z to the uint8 [n,S,S,3] `images` array of this file")
    p.add_argument("--project_steps", type=int, default=200, help="Adam updates per image")
    p.add_argument("--project_lr", type=float, default=0.05)
    p.add_argument("--project_prior", type=float, default=0.0, help="weight of mean(z^2) beside the image loss")
    p.add_argument("--score", action="store_true", help="add the discriminator's logit and prob of every image to images.npz")
    p.add_argument("--select", choices=["top", "drs"], default=None, help="keep the best / rejection-sample by the discriminator's score")
    p.add_argument("--oversample", type=int, default=None, metavar="M", help="with --select: draws per image kept (top), per round (drs)")
    p.add_argument("--score_images", default=None, metavar="FILE.npz", help="score the uint8 [n,S,S,3] `images` array of this file")
    p.add_argument("--neighbours", default=None, metavar="REF.npz", help="nearest images of this file's uint8 `images` array for every sample")
    p.add_argument("--k", type=int, default=None, help="neighbours per sample, 1..8 (default 4 with --neighbours, 5 with --probe)")
    p.add_argument("--space", choices=["pixel", "d"], default=None, help="with --neighbours: pixel space (default) or the discriminator's features")
    p.add_argument("--features", default=None, metavar="FILE.npz", help="the discriminator's pooled activations of this file's uint8 `images` array")
    p.add_argument("--feature_grid", type=int, choices=[1, 2, 4], default=None, help="with --features, --probe, --space d: the pooling raster (default 4)")
    p.add_argument("--feature_pool", choices=["max", "mean"], default=None, help="with --features, --probe, --space d (default max)")
    p.add_argument("--probe", default=None, metavar="TRAIN.npz", help="k-nearest-neighbour probe of the discriminator's features: the labelled training set")
    p.add_argument("--probe_test", default=None, metavar="TEST.npz", help="with --probe: the labelled test set")
    p.add_argument("--inpaint", default=None, metavar="FILE.npz", help="fill the holes of the uint8 [n,S,S,3] `images` array of this file")
    p.add_argument("--mask", default=None, metavar="SPEC", help="with --inpaint: center:K, half:left|right|top|bottom, or an .npz / .npy with `mask`")
    p.add_argument("--critic_weight", type=float, default=None, metavar="W", help="with --inpaint: weight of -log D(G(z)) (default 0.003; 0: no critic)")
    p.add_argument("--refine", type=int, default=None, metavar="STEPS", help="Adam updates of every latent along the discriminator's gradient")
    p.add_argument("--refine_lr", type=float, default=None, metavar="LR", help="with --refine (default 0.02)")
    p.add_argument("--project_feature_weight", type=float, default=None, metavar="W",
                   help="with --project: weight of the feature-matching term on the discriminator's deepest stage")
    p.add_argument("--anomaly", default=None, metavar="FILE.npz", help="AnoGAN anomaly scores of the uint8 [n,S,S,3] `images` array of this file")
    p.add_argument("--anomaly_lam", type=float, default=None, metavar="LAM", help="with --anomaly: weight of the feature term in the score, in [0, 1) (default 0.1)")
    p.add_argument("--anomaly_stage", type=int, default=None, metavar="K", help="with --anomaly: the discriminator stage matched (default: the deepest)")
    p.add_argument("--prec", choices=["bf16", "f32", "bf16x3"], default="bf16")
    p.add_argument("--out", required=True, help="output directory")
    a = p.parse_args(argv)
    if a.interpolate and a.num is not None:
        p.error("--interpolate PAIRS:STEPS sets the number of images; --num does not go with it")
    if a.project and (a.interpolate or a.num is not None or a.truncation is not None):
        p.error("--project takes its images from the file; --num, --interpolate and --truncation do not go with it")
    if a.project_steps < 1 or not a.project_lr > 0 or a.project_prior < 0:
        p.error("--project_steps must be >= 1, --project_lr > 0, --project_prior >= 0")
    if a.select and (a.oversample is None or a.oversample < 1):
        p.error("--select needs --oversample M with M >= 1")
    if a.oversample is not None and not a.select:
        p.error("--oversample goes with --select")
    if a.select and (a.interpolate or a.project or a.bn != "running"):
        p.error("--select draws its own latents under --bn running; --interpolate, --project and --bn batch do not go with it")
    if a.select and a.classes and len(a.classes) != 1:
        p.error("--select ranks within ONE class: give --classes a single id (scores of different classes do not compare)")
    if a.score_images and (a.interpolate or a.project or a.select or a.score or a.num is not None or a.truncation is not None):
        p.error("--score_images takes its images from the file; the sampling options do not go with it")
    if a.score and (a.project or a.bn != "running"):
        p.error("--score scores the eval-mode generator's images: not with --project or --bn batch")
    if a.neighbours and a.project:
        p.error("--neighbours looks up sampled or given images: not with --project")
    if a.space and not a.neighbours:
        p.error("--space goes with --neighbours")
    if bool(a.probe) != bool(a.probe_test):
        p.error("--probe TRAIN.npz and --probe_test TEST.npz go together")
    if a.features and a.probe:
        p.error("--features and --probe are separate runs")
    if (a.features or a.probe) and (a.interpolate or a.project or a.select or a.score or a.score_images or a.neighbours or a.inpaint or
                                    a.num is not None or a.truncation is not None or a.refine is not None):
        p.error("--features and --probe take their images from files; the sampling, projection, scoring and neighbour options do not go with them")
    if (a.feature_grid is not None or a.feature_pool is not None) and not (a.features or a.probe or a.space == "d"):
        p.error("--feature_grid and --feature_pool go with --features, --probe or --space d")
    if a.k is None:
        a.k = 5 if a.probe else 4
    if not 1 <= a.k <= 8:
        p.error("--k must lie in 1..8")
    a.space = a.space or "pixel"
    a.feature_grid = 4 if a.feature_grid is None else a.feature_grid
    a.feature_pool = a.feature_pool or "max"
    if bool(a.inpaint) != bool(a.mask):
        p.error("--inpaint FILE.npz and --mask SPEC go together")
    if a.inpaint and (a.project or a.interpolate or a.select or a.score or a.score_images or a.neighbours or a.num is not None or
                      a.truncation is not None or a.refine is not None):
        p.error("--inpaint takes its images from the file; the sampling, projection and scoring options do not go with it")
    if a.critic_weight is not None and not a.inpaint:
        p.error("--critic_weight goes with --inpaint")
    if a.critic_weight is not None and not a.critic_weight >= 0:
        p.error("--critic_weight must be >= 0")
    if a.inpaint and a.critic_weight is None:
        a.critic_weight = 0.003
    if a.project_feature_weight is not None and not a.project:
        p.error("--project_feature_weight goes with --project")
    if a.project_feature_weight is not None and not 0 <= a.project_feature_weight < float("inf"):
        p.error("--project_feature_weight must be finite and >= 0")
    if a.anomaly and (a.project or a.inpaint or a.interpolate or a.select or a.score or a.score_images or a.neighbours or a.features or a.probe or
                      a.num is not None or a.truncation is not None or a.refine is not None):
        p.error("--anomaly takes its images from the file; the sampling, projection, inpainting, scoring and feature options do not go with it")
    if (a.anomaly_lam is not None or a.anomaly_stage is not None) and not a.anomaly:
        p.error("--anomaly_lam and --anomaly_stage go with --anomaly")
    if a.anomaly_lam is not None and not 0 <= a.anomaly_lam < 1:
        p.error("--anomaly_lam must lie in [0, 1)")
    if a.anomaly_stage is not None and not -1 <= a.anomaly_stage <= 4:
        p.error("--anomaly_stage must be -1 (the deepest) or a stage of the discriminator")
    if a.anomaly and a.anomaly_lam is None:
        a.anomaly_lam = 0.1
    if a.refine_lr is not None and a.refine is None:
        p.error("--refine_lr goes with --refine")
    if a.refine is not None:
        if a.refine < 1 or (a.refine_lr is not None and not a.refine_lr > 0):
            p.error("--refine STEPS must be >= 1 and --refine_lr > 0")
        if a.project or a.score_images or a.select or a.interpolate or a.bn != "running":
            p.error("--refine moves the latents of a plain sampling run under --bn running: not with --project, --score_images, --select, --interpolate or --bn batch")
        if a.refine_lr is None:
            a.refine_lr = 0.02
    if a.num is None:
        a.num = 64
    if a.num < 1 or a.batch_size < 1 or a.calibrate < 0:
        p.error("--num and -b must be >= 1, --calibrate >= 0")
    if a.truncation is not None and not a.truncation > 0:
        p.error("--truncation must be > 0")
    if a.classes is not None and a.model != "CGAN":
        p.error("--classes needs -m CGAN")
    return a


def parse_classes(s):
    try:
        ids = [int(t) for t in s.split(",") if t.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"class ids must be integers: {s!r}")
    if not ids or min(ids) < 0 or max(ids) >= 100:
        raise argparse.ArgumentTypeError("class ids must lie in [0, 100)")
    return ids


def parse_interpolate(s):
    try:
        pairs, steps = (int(t) for t in s.split(":"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected PAIRS:STEPS, got {s!r}")
    if pairs < 1 or steps < 2:
        raise argparse.ArgumentTypeError("PAIRS >= 1 and STEPS >= 2")
    return pairs, steps


def needs_discriminator(args):
    return bool(args.score or args.select or args.score_images or args.refine is not None or (args.inpaint and args.critic_weight > 0) or
                args.features or args.probe or args.space == "d" or args.anomaly or (args.project_feature_weight or 0) > 0)


def check_checkpoint(args, ckpt):
    """Refuses, before any engine exists, a run whose flags need a discriminator the checkpoint does not have."""
    from hipgan.sampler import pick_discriminator_state
    if needs_discriminator(args):
        pick_discriminator_state(ckpt)


def plan(args):
    """(z [N,100] on the host, class ids [N] or None, images per grid row) of a run."""
    from hipgan.sampler import latents, slerp
    if args.project:
        return plan_project(args)[1:]
    if args.interpolate:
        pairs, steps = args.interpolate
        ends = latents(2 * pairs, args.seed, args.truncation)
        z = torch.cat([slerp(ends[2 * k], ends[2 * k + 1], steps) for k in range(pairs)])
        rows, per_row = pairs, steps
    elif args.classes:
        rows, per_row = len(args.classes), args.num
        z = latents(rows * per_row, args.seed, args.truncation)
    else:
        rows, per_row = None, 8
        z = latents(args.num, args.seed, args.truncation)
    cls = None
    if args.model == "CGAN":
        if args.classes:              # a class per grid row (interpolation rows cycle through the classes given)
            cls = torch.tensor([args.classes[k % len(args.classes)] for k in range(rows)]).repeat_interleave(per_row)
        else:
            cls = torch.randint(0, 100, (z.shape[0],), generator=torch.Generator().manual_seed(args.seed + 1))
    return z.float(), cls, per_row


def plan_project(args):
    """(target images uint8 [n,S,S,3], start z0 [n,100], class ids [n] or None, images per grid row) of a --project run."""
    from hipgan._lib import JckError
    from hipgan.sampler import latents, load_projection_targets
    u8, labels = load_projection_targets(args.project)
    n = u8.shape[0]
    cls = None
    if args.model == "CGAN":
        if args.classes:
            cls = torch.tensor([args.classes[k % len(args.classes)] for k in range(n)])
        elif labels is not None:
            cls = labels.to(torch.int64).view(-1)
        else:
            raise JckError(f"{args.project} has no 'labels' array: a CGAN projection needs it, or --classes")
    return u8, latents(n, args.seed), cls, min(n, 8)


def pair_rows(targets_u8, recon_u8, per_row):
    """[targets of row 0 | reconstructions of row 0 | targets of row 1 | ...], each row padded to per_row with black images: the
    order in which grid_u8 puts every target above its reconstruction."""
    t, r = np.asarray(targets_u8), np.asarray(recon_u8)
    out = []
    for lo in range(0, t.shape[0], per_row):
        for part in (t[lo:lo + per_row], r[lo:lo + per_row]):
            pad = np.zeros((per_row - part.shape[0],) + part.shape[1:], np.uint8)
            out += [part, pad]
    return np.concatenate(out)


def grid_u8(images_u8, per_row, padding=2):
    """uint8 [N,H,W,3] -> one uint8 [H',W',3] sheet, `per_row` images a row on black."""
    from train.gan_trainer import _make_grid
    x = torch.as_tensor(images_u8).permute(0, 3, 1, 2).float()
    g = _make_grid(x, nrow=per_row, padding=padding, normalize=False)
    return g.permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy()


def main(argv=None):
    args = get_arg_parse(argv)
    from hipgan.sampler import Sampler
    from train.gan_trainer import _encode_png
    with_d = needs_discriminator(args)
    ref = None
    if args.neighbours:                   # a bad reference file ends the run before an engine exists
        from hipgan.neighbours import load_reference_images
        ref = load_reference_images(args.neighbours)
    job = None
    if args.inpaint:                      # ... and so does a bad picture file or mask
        job = plan_inpaint(args)
    if args.anomaly:                      # ... or an anomaly run's file
        job = plan_anomaly(args)
    if args.features or args.probe:       # ... or a feature run's file without pictures, a probe's without labels
        from hipgan.probe import load_images
        job = [load_images(f, need_labels=bool(args.probe)) for f in ((args.features,) if args.features else (args.probe, args.probe_test))]
    ckpt = args.checkpoint
    if with_d:
        ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
        check_checkpoint(args, ckpt)
    s = Sampler.from_checkpoint(ckpt, args.model, which=args.which, prec=args.prec, batch=args.batch_size, **({"with_d": True} if with_d else {}))
    if args.calibrate:
        s.calibrate(args.calibrate, seed=args.seed + 2)
    if args.project:
        return project_main(args, s)
    if args.inpaint:
        return inpaint_main(args, s, job)
    if args.anomaly:
        return anomaly_main(args, s, job)
    if args.features:
        return features_main(args, s, job)
    if args.probe:
        return probe_main(args, s, job)
    if args.score_images:
        return score_main(args, s, ref)
    if ref is not None:                   # ... and one of the wrong size before anything is sampled
        from hipgan.neighbours import upscale_steps
        upscale_steps(ref.shape[1], s.engine.size, what=args.neighbours)
    if args.select:
        cls = None
        if args.model == "CGAN":          # one class for the whole run (--classes ID, else drawn from the seed): scores of different classes do not compare
            cls = torch.tensor(args.classes) if args.classes else torch.randint(0, 100, (1,), generator=torch.Generator().manual_seed(args.seed + 1))
        img, info = s.images(args.num, seed=args.seed, truncation=args.truncation, labels=cls, select=args.select,
                             oversample=args.oversample, return_info=True)
        u8, z, per_row, scores = img.cpu().numpy(), info["z"], 8, (info["logit"], info["prob"])
        cls = None if cls is None else cls.repeat(args.num)
    else:
        z, cls, per_row = plan(args)
        refined = None
        if args.refine is not None:       # the pictures are those of the refined latents
            zr, before, after = s.refine(z, cls, steps=args.refine, lr=args.refine_lr)
            z, refined = zr.cpu(), (before.cpu().numpy(), after.cpu().numpy())
        if args.score:                    # the scores of exactly these pictures, from the generator pass that made them
            img, *scores = s.from_latents_scored(z, cls, out="uint8")
            u8 = img.cpu().numpy()
        else:
            u8 = s.from_latents(z, cls, bn=args.bn, out="uint8").cpu().numpy()
    os.makedirs(args.out, exist_ok=True)
    arrays = {"images": u8, "z": z.numpy()}
    if cls is not None:
        arrays["labels"] = cls.numpy().astype(np.int64)
    if args.score:
        arrays["logit"], arrays["prob"] = scores[0].cpu().numpy(), scores[1].cpu().numpy()
    if args.refine is not None:
        arrays["logit_before"], arrays["logit_after"] = refined
    np.savez(os.path.join(args.out, "images.npz"), **arrays)
    with open(os.path.join(args.out, "grid.png"), "wb") as f:
        f.write(_encode_png(grid_u8(u8, per_row)))
    print(f"{u8.shape[0]} images ({s.which} generator, bn={args.bn}) -> {args.out}/images.npz, grid.png")
    if ref is not None:
        neighbours_main(args, s, u8, ref)
    return 0


def neighbours_main(args, s, u8, ref):
    """--neighbours: the samples' nearest reference images -> <out>/neighbours.npz, neighbours.png and one line"""
    from hipgan.neighbours import neighbour_rows, upscale_steps
    from train.gan_trainer import _encode_png
    steps = upscale_steps(ref.shape[1], u8.shape[1], what=args.neighbours)
    if args.space == "d":
        r = s.neighbours(u8, ref, k=args.k, space="d", grid=args.feature_grid, pool=args.feature_pool)
    else:
        r = s.neighbours(u8, ref, k=args.k)
    os.makedirs(args.out, exist_ok=True)
    np.savez(os.path.join(args.out, "neighbours.npz"), **{k_: r[k_] for k_ in ("idx", "d2", "rmse", "ref_nn_d2", "copy") if k_ in r})
    with open(os.path.join(args.out, "neighbours.png"), "wb") as f:
        f.write(_encode_png(grid_u8(neighbour_rows(u8, ref, r["idx"], steps), 1 + args.k)))
    if args.space == "d":
        near = r["d2"][:, 0]
        print(f"neighbours (discriminator features): {int(r['copy'].sum())} of {u8.shape[0]} samples flagged as copies, nearest d2 min "
              f"{float(np.nanmin(near)):.5f} median {float(np.nanmedian(near)):.5f} -> {args.out}/neighbours.npz, neighbours.png")
        return
    near = r["rmse"][:, 0]
    print(f"neighbours: {int(r['copy'].sum())} of {u8.shape[0]} samples flagged as copies, nearest rmse min {float(np.nanmin(near)):.5f} "
          f"median {float(np.nanmedian(near)):.5f} -> {args.out}/neighbours.npz, neighbours.png")


def features_main(args, s, job):
    """--features: the discriminator's pooled activations of a file's pictures -> <out>/features.npz and one line"""
    from hipgan.probe import extract, feature_layout
    (u8, labels), = job
    f = extract(s.engine, u8, args.feature_grid, args.feature_pool, normalise="none").cpu().numpy()
    layout, F = feature_layout(s.engine.size, args.feature_grid)
    arrays = {"features": f, "layout": np.asarray(layout, np.int64), "grid": np.int64(args.feature_grid), "pool": np.str_(args.feature_pool)}
    if labels is not None:
        arrays["labels"] = labels
    os.makedirs(args.out, exist_ok=True)
    np.savez(os.path.join(args.out, "features.npz"), **arrays)
    print(f"{f.shape[0]} images -> {F} features each (grid {args.feature_grid}, {args.feature_pool}) -> {args.out}/features.npz")
    return 0


def probe_main(args, s, job):
    """--probe: a k-nearest-neighbour classifier on the discriminator's features -> <out>/probe.json and one line"""
    import json
    from hipgan.probe import feature_layout
    (train, ltr), (test, lte) = job
    r = s.knn_probe(train, ltr, test, lte, k=args.k, grid=args.feature_grid, pool=args.feature_pool)
    res = {"accuracy": r["accuracy"], "per_class": {str(c): a for c, a in r["per_class"].items()}, "k": args.k, "train": int(train.shape[0]),
           "test": int(test.shape[0]), "F": feature_layout(s.engine.size, args.feature_grid)[1], "grid": args.feature_grid, "pool": args.feature_pool}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(f"probe: {res['test']} test images against {res['train']} training images, k = {args.k}, F = {res['F']}: accuracy "
          f"{res['accuracy']:.4f} -> {args.out}/probe.json")
    return 0


def score_main(args, s, ref=None):
    from hipgan._lib import JckError
    from hipgan.sampler import load_projection_targets
    u8, labels = load_projection_targets(args.score_images)
    if ref is not None:
        from hipgan.neighbours import upscale_steps
        upscale_steps(ref.shape[1], u8.shape[1], what=args.neighbours)
    cls = None
    if args.model == "CGAN":
        if args.classes:
            cls = torch.tensor([args.classes[k % len(args.classes)] for k in range(u8.shape[0])])
        elif labels is not None:
            cls = labels.to(torch.int64).view(-1)
        else:
            raise JckError(f"{args.score_images} has no 'labels' array: a CGAN discriminator needs it, or --classes")
    logit, prob = s.score(u8, cls)
    os.makedirs(args.out, exist_ok=True)
    arrays = {"logit": logit.cpu().numpy(), "prob": prob.cpu().numpy()}
    if cls is not None:
        arrays["labels"] = cls.numpy().astype(np.int64)
    np.savez(os.path.join(args.out, "scores.npz"), **arrays)
    print(f"{u8.shape[0]} images scored (mean prob {float(prob.mean()):.4f}) -> {args.out}/scores.npz")
    if ref is not None:
        neighbours_main(args, s, u8.numpy(), ref)
    return 0


def plan_inpaint(args):
    """(pictures uint8 [n,S,S,3], known bool [S,S] or [n,S,S], class ids [n] or None) of an --inpaint run; JckError for a bad file or mask"""
    from hipgan._lib import JckError
    from hipgan.inpaint import parse_mask
    from hipgan.sampler import load_projection_targets
    u8, labels = load_projection_targets(args.inpaint)
    n = u8.shape[0]
    known = parse_mask(args.mask, u8.shape[1])
    if known.dim() == 3 and known.shape[0] != n:
        raise JckError(f"{args.mask}: {known.shape[0]} masks for {n} images")
    cls = None
    if args.model == "CGAN":
        if args.classes:
            cls = torch.tensor([args.classes[k % len(args.classes)] for k in range(n)])
        elif labels is not None:
            cls = labels.to(torch.int64).view(-1)
        else:
            raise JckError(f"{args.inpaint} has no 'labels' array: a CGAN needs it, or --classes")
    return u8, known, cls


def inpaint_main(args, s, job):
    from train.gan_trainer import _encode_png
    u8, known, cls = job
    r = s.inpaint(u8, known, cls, steps=args.project_steps, lr=args.project_lr, critic_weight=args.critic_weight, seed=args.seed)
    gen, done = r["generated"].cpu().numpy(), r["completed"].cpu().numpy()
    k3 = (known if known.dim() == 3 else known.unsqueeze(0).expand(u8.shape[0], -1, -1)).numpy()
    masked = u8.numpy() * k3[..., None].astype(np.uint8)              # the holes black
    os.makedirs(args.out, exist_ok=True)
    arrays = {"z": r["z"].cpu().numpy(), "loss": r["loss"].cpu().numpy(), "term": r["term"].cpu().numpy(), "known": known.numpy(),
              "images": gen, "completed": done}
    if cls is not None:
        arrays["labels"] = cls.numpy().astype(np.int64)
    np.savez(os.path.join(args.out, "inpainted.npz"), **arrays)
    rows = np.stack([masked, gen, done], axis=1).reshape((-1,) + gen.shape[1:])      # one row per picture: masked input, G(z), completed
    with open(os.path.join(args.out, "inpainted.png"), "wb") as f:
        f.write(_encode_png(grid_u8(rows, 3)))
    print(f"{gen.shape[0]} images inpainted ({s.which} generator, {args.project_steps} steps, critic weight {args.critic_weight}, "
          f"mean loss {float(r['loss'].mean()):.5f}) -> {args.out}/inpainted.npz, inpainted.png")
    return 0


def plan_anomaly(args):
    """(pictures uint8 [n,S,S,3], class ids [n] or None, anomalous bool [n] or None) of an --anomaly run; JckError for a bad file"""
    from hipgan._lib import JckError
    from hipgan.sampler import load_projection_targets
    u8, labels = load_projection_targets(args.anomaly)
    n = u8.shape[0]
    with np.load(args.anomaly) as f:
        flags = f["anomalous"] if "anomalous" in f.files else None
    if flags is not None and (flags.dtype != np.bool_ or flags.shape != (n,)):
        raise JckError(f"{args.anomaly}: 'anomalous' must be bool [{n}], got {flags.dtype} {tuple(flags.shape)}")
    cls = None
    if args.model == "CGAN":
        if args.classes:
            cls = torch.tensor([args.classes[k % len(args.classes)] for k in range(n)])
        elif labels is not None:
            cls = labels.to(torch.int64).view(-1)
        else:
            raise JckError(f"{args.anomaly} has no 'labels' array: a CGAN needs it, or --classes")
    return u8, cls, flags


def anomaly_main(args, s, job):
    """--anomaly: AnoGAN scores of a file's pictures -> <out>/anomaly.npz, anomaly.png, anomaly.json (with flags) and one line"""
    import json
    from hipgan.anomaly import auroc
    from train.gan_trainer import _encode_png
    u8, cls, flags = job
    r = s.anomaly(u8, cls, steps=args.project_steps, lr=args.project_lr, lam=args.anomaly_lam, stage=args.anomaly_stage, seed=args.seed)
    gen, score = r["generated"].cpu().numpy(), r["score"].cpu().numpy()
    order = np.argsort(-score, kind="stable").astype(np.int64)
    os.makedirs(args.out, exist_ok=True)
    arrays = {"z": r["z"].cpu().numpy(), "residual": r["residual"].cpu().numpy(), "feature": r["feature"].cpu().numpy(), "score": score,
              "generated": gen, "order": order}
    if cls is not None:
        arrays["labels"] = cls.numpy().astype(np.int64)
    np.savez(os.path.join(args.out, "anomaly.npz"), **arrays)
    diff = np.abs(u8.numpy().astype(np.int16) - gen.astype(np.int16)).astype(np.uint8)
    rows = np.stack([u8.numpy(), gen, diff], axis=1).reshape((-1,) + gen.shape[1:])      # one row per picture: input, G(z), |input - G(z)|
    with open(os.path.join(args.out, "anomaly.png"), "wb") as f:
        f.write(_encode_png(grid_u8(rows, 3)))
    tail = ""
    if flags is not None:
        res = {"auroc": auroc(score, flags), "n": int(u8.shape[0]), "anomalous": int(flags.sum()), "lam": args.anomaly_lam,
               "stage": args.anomaly_stage}
        with open(os.path.join(args.out, "anomaly.json"), "w") as f:
            json.dump(res, f, indent=1)
        tail = f", AUROC {res['auroc']:.4f} -> anomaly.json"
    print(f"{gen.shape[0]} images scored ({s.which} generator, {args.project_steps} steps, lam {args.anomaly_lam}, mean score "
          f"{float(score.mean()):.5f}) -> {args.out}/anomaly.npz, anomaly.png{tail}")
    return 0


def project_main(args, s):
    from train.gan_trainer import _encode_png
    targets, z0, cls, per_row = plan_project(args)
    feat = {"feature_weight": args.project_feature_weight} if (args.project_feature_weight or 0) > 0 else {}
    z, loss = s.project(targets, cls, steps=args.project_steps, lr=args.project_lr, prior=args.project_prior, z0=z0, **feat)
    recon = s.from_latents(z, cls, bn="running", out="uint8").cpu().numpy()
    os.makedirs(args.out, exist_ok=True)
    arrays = {"z": z.cpu().numpy(), "loss": loss.cpu().numpy(), "images": recon}
    if cls is not None:
        arrays["labels"] = cls.numpy().astype(np.int64)
    np.savez(os.path.join(args.out, "projected.npz"), **arrays)
    with open(os.path.join(args.out, "projected.png"), "wb") as f:
        f.write(_encode_png(grid_u8(pair_rows(targets.numpy(), recon, per_row), per_row)))
    print(f"{recon.shape[0]} images projected ({s.which} generator, {args.project_steps} steps, mean loss {float(loss.mean()):.5f}) "
          f"-> {args.out}/projected.npz, projected.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
