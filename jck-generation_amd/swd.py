"""Sliced Wasserstein distance between the Laplacian-pyramid patch statistics of a trained generator's samples and the training
pictures, or of two picture files (Karras et al. 2018, section 5; the definition: DESIGN.md 5.17).  Run from inside jck-generation_amd/
like main.py:

    python swd.py -m DCGAN --checkpoint best.pt --train train.npz --num 8192 --out swd
    python swd.py -m CGAN --checkpoint best.pt --train train.npz --classes 3,17,42 --out swd3      # per class and pooled
    python swd.py --compare a/images.npz b/images.npz --out cmp                                   # two uint8 files, no checkpoint

--num samples (latents of --seed; --which ema: the averaged generator; a CGAN's classes from --classes, cycled, or drawn from the
training file's `labels`) are compared with the first --num training pictures after a permutation of that seed (--train: an .npz with
uint8 `images` [N,S,S,3], 32 x 32 data upscaled as the trainers do).  Per picture and pyramid level --patches 7 x 7 x 3 patches are
normalised per channel, projected on --repeats x --dirs random unit directions, the projections of the two sets sorted and their mean
absolute difference taken: one number per level, times 1e3, and their mean.  No metric network is involved.  How a level reads: the
finest (64x64 at a 64 x 64 generator) is the statistics of fine texture and noise, the middle one (32x32) of shapes and strokes, the
coarsest (16x16, the low-pass picture itself) of layout and colour; a run that gets the layout right and the texture wrong has a small
last number and a large first one.  Two halves of one training set against each other give the floor to compare with.  Written to --out:

    swd.json   swd (per level, x 1e3), mean, sides, levels (names), reads_as, n, n_train, seed, settings (patches, dirs, repeats) and,
               with --classes, per_class: the same per class id (its n: the smaller of the class's samples and training pictures)
    swd.npz    per_repeat [R][L] (and per_repeat_<class id>)

and one line: swd: 64x64 12.31 | 32x32 9.87 | 16x16 30.02 | mean 17.40 (8192 samples against 8192 of 50000 training pictures)

--compare A.npz[:key] B.npz[:key] takes two files of uint8 pictures of one shape (the `images` array, S in 32, 64, 128) -> swd.json and
swd.npz of A against B.  Where there is a GPU the run goes through the kernels (csrc/swd.hip), else through numpy fp64."""
import argparse
import sys

import numpy as np
import torch


def get_arg_parse(argv=None):
    from diversity import split_key
    p = argparse.ArgumentParser(description="sliced Wasserstein distance on Laplacian-pyramid patches: a trained DCGAN / CGAN generator against its "
                                            "training set, or two picture files", formatter_class=argparse.RawDescriptionHelpFormatter, epilog=__doc__)
    p.add_argument("-m", "--model", choices=["DCGAN", "CGAN"], default="DCGAN")
    p.add_argument("--checkpoint", default=None, help="a checkpoint written by the trainers (or the reference's)")
    p.add_argument("--compare", nargs=2, default=None, metavar=("A.npz[:key]", "B.npz[:key]"), help="the pictures of A against those of B")
    p.add_argument("--train", default=None, metavar="TRAIN.npz", help="the training pictures: uint8 `images` [N,S,S,3] (and `labels`)")
    p.add_argument("--num", type=int, default=8192, help="samples, and training pictures they are compared with")
    p.add_argument("--classes", default=None, help="CGAN: comma-separated class ids, cycled over the samples; one report per class plus the pooled one")
    p.add_argument("--levels", type=int, default=None, help="pyramid levels, finest first (default: every level down to 16 x 16)")
    p.add_argument("--patches", type=int, default=128, help="7 x 7 patches per picture and level")
    p.add_argument("--dirs", type=int, default=128, help="directions per repeat")
    p.add_argument("--repeats", type=int, default=4, help="repeats (fresh directions each)")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--which", choices=["auto", "live", "ema"], default="auto")
    p.add_argument("-b", "--batch_size", type=int, default=64, help="images per launch sequence")
    p.add_argument("--truncation", type=float, default=None, help="draw z from a normal truncated to [-T, T]")
    p.add_argument("--prec", choices=["bf16", "f32", "bf16x3"], default="bf16")
    a = p.parse_args(argv)
    if a.levels is not None and not 1 <= a.levels <= 4:
        p.error("--levels must lie in 1..4")
    if a.patches < 1 or a.dirs < 1 or a.repeats < 1:
        p.error("--patches, --dirs and --repeats must be >= 1")
    if a.compare:
        if a.checkpoint or a.train or a.classes:
            p.error("--compare takes two files: --checkpoint, --train and --classes do not go with it")
        a.compare = [split_key(s) for s in a.compare]
        return a
    if not a.checkpoint or not a.train:
        p.error("--checkpoint and --train are required (or --compare A.npz B.npz)")
    if a.num < 1 or a.batch_size < 1:
        p.error("--num and -b must be >= 1")
    if a.truncation is not None and not a.truncation > 0:
        p.error("--truncation must be > 0")
    if a.classes is not None:
        if a.model != "CGAN":
            p.error("--classes goes with -m CGAN")
        try:
            a.classes = [int(c) for c in a.classes.split(",")]
        except ValueError:
            p.error("--classes takes comma-separated integers")
        if not a.classes or min(a.classes) < 0 or max(a.classes) > 99:
            p.error("--classes must lie in 0..99")
    # to generate.check_checkpoint this is a plain sampling run without a discriminator
    a.mode, a.score, a.select, a.refine, a.space = "sample", False, None, None, None
    return a


def settings_of(args):
    return {"patches": args.patches, "dirs": args.dirs, "repeats": args.repeats}


def write(args, r, line):
    from generate import write_outputs
    from hipgan.swd import format_report, to_json
    record = {**to_json(r), "settings": settings_of(args), "seed": args.seed}
    arrays = {"per_repeat": r["per_repeat"]}
    if "per_class" in r:
        record["per_class"] = {str(c): to_json(v) for c, v in r["per_class"].items()}
        arrays.update({f"per_repeat_{c}": v["per_repeat"] for c, v in r["per_class"].items()})
    write_outputs(args.out, "swd.npz", arrays, record=("swd.json", record))
    print(f"swd: {format_report(r)} ({line}) -> {args.out}/swd.json, swd.npz")
    return 0


def run_compare(args):
    import metrics
    from hipgan._lib import JckError
    from hipgan.swd import SIZES
    (pa, ka), (pb, kb) = args.compare
    sets = []
    for path, key in ((pa, ka), (pb, kb)):
        with np.load(path) as f:
            if key not in f.files:
                raise JckError(f"{path}: no '{key}' array (found {sorted(f.files)})")
            x = f[key]
        if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2] or x.shape[0] < 1 or x.shape[1] not in SIZES:
            raise JckError(f"{path}: '{key}' must be uint8 [n,S,S,3] with S in {SIZES}, got {x.dtype} {tuple(x.shape)}")
        sets.append(np.ascontiguousarray(x))
    a, b = sets
    if a.shape != b.shape:
        raise JckError(f"--compare: {pa} holds {a.shape}, {pb} holds {b.shape}")
    if torch.cuda.is_available():
        a = torch.from_numpy(a).cuda()
    r = metrics.swd(a, b, levels=args.levels, seed=args.seed, **settings_of(args))
    r.update(n=int(b.shape[0]))
    return write(args, r, f"{b.shape[0]} pictures of {pa}:{ka} against {pb}:{kb}")


def main(argv=None):
    args = get_arg_parse(argv)
    if args.compare:
        return run_compare(args)
    from generate import check_checkpoint
    from hipgan.probe import load_images
    from hipgan.sampler import Sampler
    from modes import sample_classes
    train_u8, train_labels = load_images(args.train)                     # a bad file ends the run before a checkpoint is read
    if args.classes:
        cls = torch.tensor([args.classes[k % len(args.classes)] for k in range(args.num)])
    else:
        cls = sample_classes(args, train_labels, args.num)
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    check_checkpoint(args, ckpt)
    s = Sampler.from_checkpoint(ckpt, args.model, which=args.which, prec=args.prec, batch=args.batch_size)
    r = s.swd(train_u8, n=args.num, seed=args.seed, labels=cls, train_labels=train_labels if args.classes else None, truncation=args.truncation,
              classes=args.classes, levels=args.levels, **settings_of(args))
    return write(args, r, f"{r['n']} samples against {r['n']} of {r['n_train']} training pictures")


if __name__ == "__main__":
    sys.exit(main())
