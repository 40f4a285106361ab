import argparse
import json
import os
import sys
from dataclasses import dataclass, field

import numpy as np
import torch

HEAD = """Images from a trained generator, outside the trainer.  Run from this directory:

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

A run is exactly one mode: one record of MODES below, which holds the mode's arguments, defaults, checks, host-side plan, run and the
paragraph that describes it here.  The options outside the modes (-b, --seed, --bn, --which, --calibrate, --classes, --k, --project_steps,
--project_lr, --project_prior, --prec) are taken by every mode, and ignored by a mode that has no use for one.
An averaged generator (--which ema, or auto when the file has one) wants --calibrate K first: K train-mode batches that fit the
running statistics to the averaged weights (in this process only; the file is not touched).
The checkpoint's discriminator (`model_d`) is used as under Discriminator.eval(); whether its running statistics make it a good ranker,
and whether its features separate anything, is a property of the run that trained it."""


@dataclass
class Mode:
    """One kind of run.  get_arg_parse declares `arguments` in a group of the mode's own, selects the mode whose `flag` was given
    (`sample` when none was), refuses every option of another mode, runs `check` and fills in `defaults`; main calls `plan`, then `run`."""
    name: str
    doc: str                                          # the mode's paragraph of the module docstring and of --help
    arguments: tuple = ()                             # ((flag, add_argument keywords), ...): the options that go only with this mode
    flag: str = None                                  # the attribute of the selecting option; None: the run without a selector
    companions: tuple = ()                            # attributes that must come with the selector
    shares: tuple = ()                                # options of another mode's group that go with this mode too
    defaults: dict = field(default_factory=dict)      # attribute: value, or a function of args (None: leave it), where it was not given
    check: object = lambda a, p: None                 # check(args, parser): value ranges and the rules inside the mode
    needs_d: object = lambda a: True                  # needs_d(args): does this run need the checkpoint's discriminator
    plan: object = lambda a: None                     # plan(args): host only; reads and checks the run's files -> job; JckError for a bad one
    run: object = None                                # run(args, sampler, job)

    def options(self):
        return tuple(flag.lstrip("-") for flag, _ in self.arguments) + tuple(self.shares)

    def title(self):
        return f"--{self.flag}" if self.flag else "a sampling run"


# what an option that no mode set rests at, in every mode
RESTING = {"num": 64, "k": 4, "space": "pixel", "feature_grid": 4, "feature_pool": "max"}


def _given(a, name):
    v = getattr(a, name)
    return v is not None and v is not False and v != ""


def get_arg_parse(argv=None):
    p = argparse.ArgumentParser(description="sample a trained DCGAN / CGAN generator", formatter_class=argparse.RawDescriptionHelpFormatter,
                                epilog="\n".join(m.doc for m in MODES))
    p.add_argument("-m", "--model", choices=["DCGAN", "CGAN"], default="DCGAN")
    p.add_argument("--checkpoint", required=True, help="a checkpoint written by the trainers (or the reference's)")
    p.add_argument("-b", "--batch_size", type=int, default=64, help="images per launch sequence")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--bn", choices=["running", "batch"], default="running")
    p.add_argument("--which", choices=["auto", "live", "ema"], default="auto")
    p.add_argument("--calibrate", type=int, default=0, metavar="K", help="train-mode sampling batches before sampling")
    p.add_argument("--classes", type=parse_classes, default=None, metavar="3,17,...", help="CGAN: one grid row of --num images per class")
    p.add_argument("--k", type=int, default=None, help="neighbours per sample, 1..8 (default 4 with --neighbours, 5 with --probe)")
    p.add_argument("--project_steps", type=int, default=200, help="Adam updates per image")
    p.add_argument("--project_lr", type=float, default=0.05)
    p.add_argument("--project_prior", type=float, default=0.0, help="weight of mean(z^2) beside the image loss")
    p.add_argument("--prec", choices=["bf16", "f32", "bf16x3"], default="bf16")
    p.add_argument("--out", required=True, help="output directory")
    for m in MODES:
        g = p.add_argument_group(f"{m.name} ({m.title()})")
        for flag, kw in m.arguments:
            g.add_argument(flag, **{"default": None, **kw})
    a = p.parse_args(argv)
    picked = [m for m in MODES if m.flag and _given(a, m.flag)]
    if len(picked) > 1:
        p.error(f"{' and '.join(m.title() for m in picked)} are separate runs")
    mode = picked[0] if picked else next(m for m in MODES if m.flag is None)
    for c in mode.companions:
        if not _given(a, c):
            p.error(f"--{mode.flag} and --{c} go together")
    homes = {}                            # option: the modes it goes with
    for m in MODES:
        for o in m.options():
            homes.setdefault(o, []).append(m)
    for o, ms in homes.items():
        if _given(a, o) and mode not in ms:
            p.error(f"--{o} goes with {' or '.join(m.title() for m in ms)}, not with {mode.title()}")
    if a.project_steps < 1 or not a.project_lr > 0 or a.project_prior < 0:
        p.error("--project_steps must be >= 1, --project_lr > 0, --project_prior >= 0")
    if a.k is not None and not 1 <= a.k <= 8:
        p.error("--k must lie in 1..8")
    if a.batch_size < 1 or a.calibrate < 0:
        p.error("-b must be >= 1, --calibrate >= 0")
    if a.classes is not None and a.model != "CGAN":
        p.error("--classes needs -m CGAN")
    mode.check(a, p)
    for name, v in {**RESTING, **mode.defaults}.items():
        if getattr(a, name) is None:
            setattr(a, name, v(a) if callable(v) else v)
    a.mode = mode.name
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


def mode_of(args):
    return next(m for m in MODES if m.name == args.mode)


def needs_discriminator(args):
    return bool(mode_of(args).needs_d(args))


def check_checkpoint(args, ckpt):
    """Refuses, before any engine exists, a run whose flags need a discriminator the checkpoint does not have."""
    from hipgan.sampler import pick_discriminator_state
    if needs_discriminator(args):
        pick_discriminator_state(ckpt)


def class_ids(args, n, labels, path):
    """Class ids [n] of a run on the n pictures of file `path` (None for a DCGAN): --classes cycled, else the file's `labels`"""
    from hipgan._lib import JckError
    if args.model != "CGAN":
        return None
    if args.classes:
        return torch.tensor([args.classes[k % len(args.classes)] for k in range(n)])
    if labels is None:
        raise JckError(f"{path} has no 'labels' array: a CGAN needs it, or --classes")
    return labels.to(torch.int64).view(-1)


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


def write_outputs(out, npz=None, arrays=None, cls=None, sheet=None, record=None):
    """A run's files in directory `out`: `npz` of `arrays` (and `labels` where there are class ids), sheet = (uint8 images, images per
    row, .png name) through grid_u8, record = (.json name, dict)."""
    from train.gan_trainer import _encode_png
    os.makedirs(out, exist_ok=True)
    if npz:
        if cls is not None:
            arrays = {**arrays, "labels": cls.numpy().astype(np.int64)}
        np.savez(os.path.join(out, npz), **arrays)
    if sheet:
        images, per_row, png = sheet
        with open(os.path.join(out, png), "wb") as f:
            f.write(_encode_png(grid_u8(images, per_row)))
    if record:
        with open(os.path.join(out, record[0]), "w") as f:
            json.dump(record[1], f, indent=1)


def check_lookup(a, p):
    """the rules of --neighbours and its options, for the two modes that take it"""
    if a.space and not a.neighbours:
        p.error("--space goes with --neighbours")
    if (a.feature_grid is not None or a.feature_pool is not None) and a.space != "d":
        p.error("--feature_grid and --feature_pool go with --features, --probe or --space d")


def check_sample(a, p):
    if a.interpolate and a.num is not None:
        p.error("--interpolate PAIRS:STEPS sets the number of images; --num does not go with it")
    if (a.num is not None and a.num < 1) or (a.truncation is not None and not a.truncation > 0):
        p.error("--num must be >= 1, --truncation > 0")
    if a.select and (a.oversample is None or a.oversample < 1):
        p.error("--select needs --oversample M with M >= 1")
    if a.oversample is not None and not a.select:
        p.error("--oversample goes with --select")
    if a.select and (a.interpolate or a.bn != "running"):
        p.error("--select draws its own latents under --bn running; --interpolate and --bn batch do not go with it")
    if a.select and a.classes and len(a.classes) != 1:
        p.error("--select ranks within ONE class: give --classes a single id (scores of different classes do not compare)")
    if a.score and a.bn != "running":
        p.error("--score scores the eval-mode generator's images: not with --bn batch")
    if a.refine_lr is not None and a.refine is None:
        p.error("--refine_lr goes with --refine")
    if a.refine is not None:
        if a.refine < 1 or (a.refine_lr is not None and not a.refine_lr > 0):
            p.error("--refine STEPS must be >= 1 and --refine_lr > 0")
        if a.select or a.interpolate or a.bn != "running":
            p.error("--refine moves the latents of a plain sampling run under --bn running: not with --select, --interpolate or --bn batch")
    check_lookup(a, p)


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


def load_reference(args):
    """the pictures of --neighbours REF.npz, or None: a bad reference file ends the run before an engine exists"""
    from hipgan.neighbours import load_reference_images
    return load_reference_images(args.neighbours) if args.neighbours else None


def plan_sample(args):
    """(plan(args), or None for --select, whose latents Sampler.images draws; the reference pictures of --neighbours or None)"""
    return None if args.select else plan(args), load_reference(args)


def run_sample(args, s, job):
    planned, ref = job
    if ref is not None:                   # a reference of the wrong size ends the run before anything is sampled
        from hipgan.neighbours import upscale_steps
        upscale_steps(ref.shape[1], s.engine.size, what=args.neighbours)
    more = {}
    if args.select:
        cls = None
        if args.model == "CGAN":          # one class for the whole run (--classes ID, else drawn from the seed): scores of different classes do not compare
            cls = torch.tensor(args.classes) if args.classes else torch.randint(0, 100, (1,), generator=torch.Generator().manual_seed(args.seed + 1))
        img, info = s.images(args.num, seed=args.seed, truncation=args.truncation, labels=cls, select=args.select,
                             oversample=args.oversample, return_info=True)
        u8, z, per_row, scores = img.cpu().numpy(), info["z"], 8, (info["logit"], info["prob"])
        cls = None if cls is None else cls.repeat(args.num)
    else:
        z, cls, per_row = planned
        if args.refine is not None:       # the pictures are those of the refined latents
            zr, before, after = s.refine(z, cls, steps=args.refine, lr=args.refine_lr)
            z, more = zr.cpu(), {"logit_before": before.cpu().numpy(), "logit_after": after.cpu().numpy()}
        if args.score:                    # the scores of exactly these pictures, from the generator pass that made them
            img, *scores = s.from_latents_scored(z, cls, out="uint8")
            u8 = img.cpu().numpy()
        else:
            u8 = s.from_latents(z, cls, bn=args.bn, out="uint8").cpu().numpy()
    if args.score:
        more.update(logit=scores[0].cpu().numpy(), prob=scores[1].cpu().numpy())
    write_outputs(args.out, "images.npz", {"images": u8, "z": z.numpy(), **more}, cls, sheet=(u8, per_row, "grid.png"))
    print(f"{u8.shape[0]} images ({s.which} generator, bn={args.bn}) -> {args.out}/images.npz, grid.png")
    if ref is not None:
        write_neighbours(args, s, u8, ref)


def write_neighbours(args, s, u8, ref):
    """--neighbours: the samples' nearest reference images -> <out>/neighbours.npz, neighbours.png and one line"""
    from hipgan.neighbours import neighbour_rows, upscale_steps
    steps = upscale_steps(ref.shape[1], u8.shape[1], what=args.neighbours)
    if args.space == "d":
        r = s.neighbours(u8, ref, k=args.k, space="d", grid=args.feature_grid, pool=args.feature_pool)
    else:
        r = s.neighbours(u8, ref, k=args.k)
    write_outputs(args.out, "neighbours.npz", {k_: r[k_] for k_ in ("idx", "d2", "rmse", "ref_nn_d2", "copy") if k_ in r},
                  sheet=(neighbour_rows(u8, ref, r["idx"], steps), 1 + args.k, "neighbours.png"))
    if args.space == "d":
        near = r["d2"][:, 0]
        print(f"neighbours (discriminator features): {int(r['copy'].sum())} of {u8.shape[0]} samples flagged as copies, nearest d2 min "
              f"{float(np.nanmin(near)):.5f} median {float(np.nanmedian(near)):.5f} -> {args.out}/neighbours.npz, neighbours.png")
        return
    near = r["rmse"][:, 0]
    print(f"neighbours: {int(r['copy'].sum())} of {u8.shape[0]} samples flagged as copies, nearest rmse min {float(np.nanmin(near)):.5f} "
          f"median {float(np.nanmedian(near)):.5f} -> {args.out}/neighbours.npz, neighbours.png")


SAMPLE = Mode(
    name="sample",
    doc="""sample (no selecting option): writes <out>/images.npz (images: uint8 [N,S,S,3]; z: fp32 [N,100]; labels: int64 class ids [N], CGAN
only) and <out>/grid.png.  BatchNorm runs on the running statistics by default (--bn running): every image is a function of its own z,
and --num is not bounded by the batch.  --bn batch is the trainers' evaluation sampling: each chunk of -b images is one train-mode
BatchNorm batch.
--score adds the discriminator's `logit` and `prob` fp32 [N] to images.npz; --select top|drs with --oversample M keeps the --num best of
M * --num draws, or runs discriminator rejection sampling with rounds of that size (Sampler.images; a CGAN ranks within one class:
--classes ID, else one drawn from the seed).
--refine STEPS moves every latent STEPS Adam updates (--refine_lr) along the discriminator's gradient before its image is made;
images.npz then holds the refined z and gains logit_before / logit_after.
--neighbours REF.npz (here, or with --score_images, whose images it then takes) looks up the --k nearest images of REF's uint8 `images`
array (the samples' size, or 32x32 training data, upscaled as the trainers do) for every sample, in pixel space: <out>/neighbours.npz
(idx int64 [n,k]; d2 squared distance in [-1, 1] units; rmse = sqrt(d2 / D); ref_nn_d2: the nearest other reference image's d2 from
the image idx[:,0]; copy = d2[:,0] < ref_nn_d2) and <out>/neighbours.png, each sample followed by its neighbours.  --space d looks the
neighbours up in the discriminator's block-normalised feature space (--feature_grid, --feature_pool) instead: neighbours.npz then
holds idx, d2, ref_nn_d2 and copy, no rmse.""",
    arguments=(
        ("--num", dict(type=int, help="images, per class with --classes (default 64; not with --interpolate)")),
        ("--truncation", dict(type=float, help="draw z from a normal truncated to [-T, T]")),
        ("--interpolate", dict(type=parse_interpolate, metavar="PAIRS:STEPS",
                               help="PAIRS spherical interpolations of STEPS points each between random z (one grid row per pair)")),
        ("--score", dict(action="store_true", default=False, help="add the discriminator's logit and prob of every image to images.npz")),
        ("--select", dict(choices=["top", "drs"], help="keep the best / rejection-sample by the discriminator's score")),
        ("--oversample", dict(type=int, metavar="M", help="with --select: draws per image kept (top), per round (drs)")),
        ("--refine", dict(type=int, metavar="STEPS", help="Adam updates of every latent along the discriminator's gradient")),
        ("--refine_lr", dict(type=float, metavar="LR", help="with --refine (default 0.02)")),
        ("--neighbours", dict(metavar="REF.npz", help="nearest images of this file's uint8 `images` array for every sample")),
        ("--space", dict(choices=["pixel", "d"], help="with --neighbours: pixel space (default) or the discriminator's features"))),
    shares=("feature_grid", "feature_pool"),
    defaults={"refine_lr": lambda a: None if a.refine is None else 0.02},
    check=check_sample,
    needs_d=lambda a: a.score or a.select or a.refine is not None or a.space == "d",
    plan=plan_sample,
    run=run_sample)


def check_project(a, p):
    if a.project_feature_weight is not None and not 0 <= a.project_feature_weight < float("inf"):
        p.error("--project_feature_weight must be finite and >= 0")


def plan_project(args):
    """(target images uint8 [n,S,S,3], start z0 [n,100], class ids [n] or None, images per grid row) of a --project run."""
    from hipgan.sampler import latents, load_projection_targets
    u8, labels = load_projection_targets(args.project)
    n = u8.shape[0]
    return u8, latents(n, args.seed), class_ids(args, n, labels, args.project), min(n, 8)


def run_project(args, s, job):
    targets, z0, cls, per_row = job
    feat = {"feature_weight": args.project_feature_weight} if (args.project_feature_weight or 0) > 0 else {}
    z, loss = s.project(targets, cls, steps=args.project_steps, lr=args.project_lr, prior=args.project_prior, z0=z0, **feat)
    recon = s.from_latents(z, cls, bn="running", out="uint8").cpu().numpy()
    write_outputs(args.out, "projected.npz", {"z": z.cpu().numpy(), "loss": loss.cpu().numpy(), "images": recon}, cls,
                  sheet=(pair_rows(targets.numpy(), recon, per_row), per_row, "projected.png"))
    print(f"{recon.shape[0]} images projected ({s.which} generator, {args.project_steps} steps, mean loss {float(loss.mean()):.5f}) "
          f"-> {args.out}/projected.npz, projected.png")


PROJECT = Mode(
    name="project", flag="project",
    doc="""--project FILE.npz fits a latent to every picture of the file's `images` array (uint8 [n,S,S,3]: an images.npz of this tool, or any
such array; a CGAN takes the file's `labels` or cycles through --classes) by Adam through the frozen eval-mode generator
(--project_steps, --project_lr, --project_prior) and writes <out>/projected.npz (z: fp32 [n,100]; loss: the mean squared error of each
reconstruction in [-1, 1] units; images: the reconstructions, uint8) and <out>/projected.png, each row of targets above the row of
their reconstructions.  --project_feature_weight W adds W times the mean squared distance between the discriminator's deepest-stage
activations of G(z) and of the picture to the objective (perceptual projection; needs `model_d`).""",
    arguments=(
        ("--project", dict(metavar="FILE.npz", help="fit z to the uint8 [n,S,S,3] `images` array of this file")),
        ("--project_feature_weight", dict(type=float, metavar="W",
                                          help="with --project: weight of the feature-matching term on the discriminator's deepest stage"))),
    check=check_project,
    needs_d=lambda a: (a.project_feature_weight or 0) > 0,
    plan=plan_project,
    run=run_project)


def check_inpaint(a, p):
    if a.critic_weight is not None and not a.critic_weight >= 0:
        p.error("--critic_weight must be >= 0")


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
    return u8, known, class_ids(args, n, labels, args.inpaint)


def run_inpaint(args, s, job):
    u8, known, cls = job
    r = s.inpaint(u8, known, cls, steps=args.project_steps, lr=args.project_lr, critic_weight=args.critic_weight, seed=args.seed)
    gen, done = r["generated"].cpu().numpy(), r["completed"].cpu().numpy()
    k3 = (known if known.dim() == 3 else known.unsqueeze(0).expand(u8.shape[0], -1, -1)).numpy()
    masked = u8.numpy() * k3[..., None].astype(np.uint8)              # the holes black
    arrays = {"z": r["z"].cpu().numpy(), "loss": r["loss"].cpu().numpy(), "term": r["term"].cpu().numpy(), "known": known.numpy(),
              "images": gen, "completed": done}
    rows = np.stack([masked, gen, done], axis=1).reshape((-1,) + gen.shape[1:])      # one row per picture: masked input, G(z), completed
    write_outputs(args.out, "inpainted.npz", arrays, cls, sheet=(rows, 3, "inpainted.png"))
    print(f"{gen.shape[0]} images inpainted ({s.which} generator, {args.project_steps} steps, critic weight {args.critic_weight}, "
          f"mean loss {float(r['loss'].mean()):.5f}) -> {args.out}/inpainted.npz, inpainted.png")


INPAINT = Mode(
    name="inpaint", flag="inpaint", companions=("mask",),
    doc="""--inpaint FILE.npz --mask SPEC is semantic inpainting (Yeh et al. 2017; Sampler.inpaint): SPEC names the KNOWN pixels of the file's
pictures ("center:K": a centred K x K hole; "half:left|right|top|bottom": that half is the hole; an .npz / .npy file holding `mask`),
z is fitted to them alone (--project_steps, --project_lr) with --critic_weight W times -log D(G(z)) as the realism prior (0: none, no
discriminator needed), and <out>/inpainted.npz holds z, loss, term, known, images (G(z)) and completed (the known pixels of the input,
the holes from G); <out>/inpainted.png has one row per picture: masked input, G(z), completed.""",
    arguments=(
        ("--inpaint", dict(metavar="FILE.npz", help="fill the holes of the uint8 [n,S,S,3] `images` array of this file")),
        ("--mask", dict(metavar="SPEC", help="with --inpaint: center:K, half:left|right|top|bottom, or an .npz / .npy with `mask`")),
        ("--critic_weight", dict(type=float, metavar="W", help="with --inpaint: weight of -log D(G(z)) (default 0.003; 0: no critic)"))),
    defaults={"critic_weight": 0.003},
    check=check_inpaint,
    needs_d=lambda a: a.critic_weight > 0,
    plan=plan_inpaint,
    run=run_inpaint)


def check_anomaly(a, p):
    if a.anomaly_lam is not None and not 0 <= a.anomaly_lam < 1:
        p.error("--anomaly_lam must lie in [0, 1)")
    if a.anomaly_stage is not None and not -1 <= a.anomaly_stage <= 4:
        p.error("--anomaly_stage must be -1 (the deepest) or a stage of the discriminator")


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
    return u8, class_ids(args, n, labels, args.anomaly), flags


def run_anomaly(args, s, job):
    from hipgan.anomaly import auroc
    u8, cls, flags = job
    r = s.anomaly(u8, cls, steps=args.project_steps, lr=args.project_lr, lam=args.anomaly_lam, stage=args.anomaly_stage, seed=args.seed)
    gen, score = r["generated"].cpu().numpy(), r["score"].cpu().numpy()
    order = np.argsort(-score, kind="stable").astype(np.int64)
    arrays = {"z": r["z"].cpu().numpy(), "residual": r["residual"].cpu().numpy(), "feature": r["feature"].cpu().numpy(), "score": score,
              "generated": gen, "order": order}
    diff = np.abs(u8.numpy().astype(np.int16) - gen.astype(np.int16)).astype(np.uint8)
    rows = np.stack([u8.numpy(), gen, diff], axis=1).reshape((-1,) + gen.shape[1:])      # one row per picture: input, G(z), |input - G(z)|
    res, tail = None, ""
    if flags is not None:
        res = {"auroc": auroc(score, flags), "n": int(u8.shape[0]), "anomalous": int(flags.sum()), "lam": args.anomaly_lam,
               "stage": args.anomaly_stage}
        tail = f", AUROC {res['auroc']:.4f} -> anomaly.json"
    write_outputs(args.out, "anomaly.npz", arrays, cls, sheet=(rows, 3, "anomaly.png"), record=res and ("anomaly.json", res))
    print(f"{gen.shape[0]} images scored ({s.which} generator, {args.project_steps} steps, lam {args.anomaly_lam}, mean score "
          f"{float(score.mean()):.5f}) -> {args.out}/anomaly.npz, anomaly.png{tail}")


ANOMALY = Mode(
    name="anomaly", flag="anomaly",
    doc="""--anomaly FILE.npz scores the file's pictures after AnoGAN (Schlegl et al. 2017; Sampler.anomaly): each is projected (--project_steps,
--project_lr) with a residual term and a feature-matching term on the discriminator's stage --anomaly_stage (default: the deepest),
and score = (1 - lam) residual + lam feature at the z reached (--anomaly_lam, default 0.1) - mean squared forms, not the paper's L1
sums.  <out>/anomaly.npz holds z, residual, feature, score, generated (G(z), uint8) and order (indices by falling score);
<out>/anomaly.png has one row per picture: input, G(z), |input - G(z)|; <out>/anomaly.json (auroc, n, anomalous, lam, stage) is written
when the file carries a bool `anomalous` [n] array.""",
    arguments=(
        ("--anomaly", dict(metavar="FILE.npz", help="AnoGAN anomaly scores of the uint8 [n,S,S,3] `images` array of this file")),
        ("--anomaly_lam", dict(type=float, metavar="LAM", help="with --anomaly: weight of the feature term in the score, in [0, 1) (default 0.1)")),
        ("--anomaly_stage", dict(type=int, metavar="K", help="with --anomaly: the discriminator stage matched (default: the deepest)"))),
    defaults={"anomaly_lam": 0.1},
    check=check_anomaly,
    plan=plan_anomaly,
    run=run_anomaly)


def plan_feature_files(args):
    """[(pictures uint8 [n,S,S,3], labels or None)] of a --features run's file, or of a --probe run's two, which must both have labels"""
    from hipgan.probe import load_images
    return [load_images(f, need_labels=bool(args.probe)) for f in ((args.features,) if args.features else (args.probe, args.probe_test))]


def run_features(args, s, job):
    from hipgan.probe import extract, feature_layout
    (u8, labels), = job
    f = extract(s.engine, u8, args.feature_grid, args.feature_pool, normalise="none").cpu().numpy()
    layout, F = feature_layout(s.engine.size, args.feature_grid)
    arrays = {"features": f, "layout": np.asarray(layout, np.int64), "grid": np.int64(args.feature_grid), "pool": np.str_(args.feature_pool)}
    if labels is not None:                # the file's labels as they are, for a DCGAN too
        arrays["labels"] = labels
    write_outputs(args.out, "features.npz", arrays)
    print(f"{f.shape[0]} images -> {F} features each (grid {args.feature_grid}, {args.feature_pool}) -> {args.out}/features.npz")


FEATURES = Mode(
    name="features", flag="features",
    doc="""The discriminator as a feature extractor (Radford et al. 2016, section 5.1; hipgan.probe): --features FILE.npz pools every conv stage's
activation of the file's pictures (the discriminator's size, or 32x32 data, upscaled as the trainers do) to a --feature_grid raster
(--feature_pool max|mean) and writes <out>/features.npz (features: fp32 [n,F], unnormalised; layout: int64 [stages,4] rows of stage,
col0, C, H; grid; pool; labels if the file has them) for an external classifier.""",
    arguments=(
        ("--features", dict(metavar="FILE.npz", help="the discriminator's pooled activations of this file's uint8 `images` array")),
        ("--feature_grid", dict(type=int, choices=[1, 2, 4], help="with --features, --probe, --space d: the pooling raster (default 4)")),
        ("--feature_pool", dict(choices=["max", "mean"], help="with --features, --probe, --space d (default max)"))),
    plan=plan_feature_files,
    run=run_features)


def run_probe(args, s, job):
    from hipgan.probe import feature_layout
    (train, ltr), (test, lte) = job
    r = s.knn_probe(train, ltr, test, lte, k=args.k, grid=args.feature_grid, pool=args.feature_pool)
    res = {"accuracy": r["accuracy"], "per_class": {str(c): a for c, a in r["per_class"].items()}, "k": args.k, "train": int(train.shape[0]),
           "test": int(test.shape[0]), "F": feature_layout(s.engine.size, args.feature_grid)[1], "grid": args.feature_grid, "pool": args.feature_pool}
    write_outputs(args.out, record=("probe.json", res))
    print(f"probe: {res['test']} test images against {res['train']} training images, k = {args.k}, F = {res['F']}: accuracy "
          f"{res['accuracy']:.4f} -> {args.out}/probe.json")


PROBE = Mode(
    name="probe", flag="probe", companions=("probe_test",),
    doc="""--probe TRAIN.npz --probe_test TEST.npz (both with `labels`) classifies every test picture by the majority of its --k (default 5)
nearest training pictures in block-normalised feature space (--feature_grid, --feature_pool) and writes <out>/probe.json (accuracy,
per_class, k, train, test, F, grid, pool).""",
    arguments=(
        ("--probe", dict(metavar="TRAIN.npz", help="k-nearest-neighbour probe of the discriminator's features: the labelled training set")),
        ("--probe_test", dict(metavar="TEST.npz", help="with --probe: the labelled test set"))),
    shares=("feature_grid", "feature_pool"),
    defaults={"k": 5},
    plan=plan_feature_files,
    run=run_probe)


def plan_score_images(args):
    """(pictures uint8 [n,S,S,3], class ids [n] or None, the reference pictures of --neighbours or None)"""
    from hipgan.sampler import load_projection_targets
    ref = load_reference(args)
    u8, labels = load_projection_targets(args.score_images)
    if ref is not None:
        from hipgan.neighbours import upscale_steps
        upscale_steps(ref.shape[1], u8.shape[1], what=args.neighbours)
    return u8, class_ids(args, u8.shape[0], labels, args.score_images), ref


def run_score_images(args, s, job):
    u8, cls, ref = job
    logit, prob = s.score(u8, cls)
    write_outputs(args.out, "scores.npz", {"logit": logit.cpu().numpy(), "prob": prob.cpu().numpy()}, cls)
    print(f"{u8.shape[0]} images scored (mean prob {float(prob.mean()):.4f}) -> {args.out}/scores.npz")
    if ref is not None:
        write_neighbours(args, s, u8.numpy(), ref)


SCORE_IMAGES = Mode(
    name="score_images", flag="score_images",
    doc="""--score_images FILE.npz scores an existing uint8 `images` array into <out>/scores.npz (logit, prob: fp32 [n]; labels for a CGAN);
--neighbours REF.npz then looks up the neighbours of these pictures, as in a sampling run.""",
    arguments=(("--score_images", dict(metavar="FILE.npz", help="score the uint8 [n,S,S,3] `images` array of this file")),),
    shares=("neighbours", "space", "feature_grid", "feature_pool"),
    check=check_lookup,
    plan=plan_score_images,
    run=run_score_images)


MODES = [SAMPLE, PROJECT, INPAINT, ANOMALY, FEATURES, PROBE, SCORE_IMAGES]
__doc__ = HEAD + "\n" + "\n".join(m.doc for m in MODES)


def main(argv=None):
    args = get_arg_parse(argv)
    from hipgan.sampler import Sampler
    mode = mode_of(args)
    job = mode.plan(args)                 # a bad file ends the run before a checkpoint is read or an engine exists
    with_d = needs_discriminator(args)
    ckpt = args.checkpoint
    if with_d:
        ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
        check_checkpoint(args, ckpt)
    s = Sampler.from_checkpoint(ckpt, args.model, which=args.which, prec=args.prec, batch=args.batch_size, **({"with_d": True} if with_d else {}))
    if args.calibrate:
        s.calibrate(args.calibrate, seed=args.seed + 2)
    mode.run(args, s, job)
    return 0


if __name__ == "__main__":
    sys.exit(main())
