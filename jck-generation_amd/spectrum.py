"""Power spectra of a trained generator's samples against the training pictures', or of two picture files (Odena et al. 2016; Durall et
al. 2020; Dzanic et al. 2020; the definition: DESIGN.md 5.18).  Run from inside jck-generation_amd/ like main.py:

    python spectrum.py -m DCGAN --checkpoint best.pt --train train.npz --num 8192 --out spectrum
    python spectrum.py --compare a/images.npz b/images.npz --out cmp                               # two uint8 files, no checkpoint

--num samples (latents of --seed; --which ema: the averaged generator; a CGAN's classes from --classes, cycled, or drawn from the
training file's `labels`) are compared with the first --num training pictures after a permutation of that seed (--train: an .npz with
uint8 `images` [N,S,S,3], 32 x 32 data upscaled as the trainers do).  Of every picture one plane (--plane luma | r | g | b) is centred,
optionally windowed (--window hann: removes the leakage of the borders), transformed, and its power averaged over rings of integer radius:
R = 24 / 46 / 92 numbers per picture at S = 32 / 64 / 128, in byte levels squared.  How the report reads: gap_db[r] is the samples' mean
log power minus the training set's at radius r - a stack of stride-2 transposed convolutions typically bends away at high radius
(high_gap_db) and leaves peaks at the lattice frequencies (a S/4, b S/4); the one at (S/2, S/2) is the checkerboard (checkerboard_db, the
samples' peak over its neighbourhood minus the training set's, in dB).  separability is the AUROC of a linear rule on the R numbers fitted
on half of the pictures: 0.5 = the spectra do not tell the sets apart.  Written to --out:

    spectrum.json   rms_gap_db, high_gap_db, worst (bin, gap_db, z), peaks (15 lattice points: a_db, b_db, diff_db), checkerboard_db,
                    separability, S, plane, window, bins, n_a, n_b (n, n_train, seed) and, with --classes, per_class: the same per class id
    spectrum.npz    radius, count, mean_db_a / std_db_a (samples), mean_db_b / std_db_b (training pictures), gap_db, z, mean2d_a, mean2d_b
                    (with --classes also <name>_<class id>)
    spectrum.png    one sheet: the samples' mean spectrum, the training set's (10 log10 over -20 .. 50 dB, zero frequency at the centre)
                    and their difference in dB (-10 .. +10; red: the samples have more, blue: less)

--compare A.npz[:key] B.npz[:key] takes two files of uint8 pictures of one S (the `images` array, S in 32, 64, 128; the counts may
differ) -> the same three files for A against B.  Where there is a GPU the run goes through the kernel (csrc/spectrum.hip), else through
numpy fp64."""
import argparse
import sys

import numpy as np
import torch


def get_arg_parse(argv=None):
    from diversity import split_key
    p = argparse.ArgumentParser(description="power spectra (radial profiles, lattice peaks) of a trained DCGAN / CGAN generator's samples against its "
                                            "training set, or of two picture files", formatter_class=argparse.RawDescriptionHelpFormatter, epilog=__doc__)
    p.add_argument("-m", "--model", choices=["DCGAN", "CGAN"], default="DCGAN")
    p.add_argument("--checkpoint", default=None, help="a checkpoint written by the trainers (or the reference's)")
    p.add_argument("--compare", nargs=2, default=None, metavar=("A.npz[:key]", "B.npz[:key]"), help="the pictures of A against those of B")
    p.add_argument("--train", default=None, metavar="TRAIN.npz", help="the training pictures: uint8 `images` [N,S,S,3] (and `labels`)")
    p.add_argument("--num", type=int, default=8192, help="samples, and training pictures they are compared with")
    p.add_argument("--classes", default=None, help="CGAN: comma-separated class ids, cycled over the samples; one report per class plus the pooled one")
    p.add_argument("--plane", choices=["luma", "r", "g", "b"], default="luma")
    p.add_argument("--window", choices=["hann"], default=None, help="periodic Hann window in both axes (default: none)")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--which", choices=["auto", "live", "ema"], default="auto")
    p.add_argument("-b", "--batch_size", type=int, default=64, help="images per launch sequence")
    p.add_argument("--truncation", type=float, default=None, help="draw z from a normal truncated to [-T, T]")
    p.add_argument("--prec", choices=["bf16", "f32", "bf16x3"], default="bf16")
    a = p.parse_args(argv)
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
    return {"plane": args.plane, "window": args.window}


def sheet_of(r):
    """uint8 [3][S][S][3]: the samples' mean spectrum, the training set's, their dB difference"""
    from hipgan.spectrum import render, render_diff
    return np.stack([render(r["mean2d_a"]), render(r["mean2d_b"]), render_diff(r["mean2d_a"], r["mean2d_b"])])


def write(args, r, line):
    from generate import write_outputs
    from hipgan.spectrum import arrays_of, format_report, to_json
    record = to_json(r)
    arrays = arrays_of(r)
    if "per_class" in r:
        record["per_class"] = {str(c): to_json(v) for c, v in r["per_class"].items()}
        for c, v in r["per_class"].items():
            arrays.update(arrays_of(v, f"_{c}"))
    write_outputs(args.out, "spectrum.npz", arrays, sheet=(sheet_of(r), 3, "spectrum.png"), record=("spectrum.json", record))
    print(f"spectrum: {format_report(r)} ({line}) -> {args.out}/spectrum.json, spectrum.npz, spectrum.png")
    return 0


def run_compare(args):
    import metrics
    from hipgan._lib import JckError
    from hipgan.spectrum import SIZES
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
    if a.shape[1:] != b.shape[1:]:
        raise JckError(f"--compare: {pa} holds {a.shape}, {pb} holds {b.shape}")
    if torch.cuda.is_available():
        a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    kw = dict(mean2d=True, **settings_of(args))
    r = metrics.spectrum_report(metrics.spectrum(a, **kw), metrics.spectrum(b, **kw))
    return write(args, r, f"{a.shape[0]} pictures of {pa}:{ka} against {b.shape[0]} of {pb}:{kb}")


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
    r = s.spectrum(train_u8, n=args.num, seed=args.seed, labels=cls, train_labels=train_labels if args.classes else None, truncation=args.truncation,
                   classes=args.classes, **settings_of(args))
    return write(args, r, f"{r['n']} samples against {r['n']} of {r['n_train']} training pictures")


if __name__ == "__main__":
    sys.exit(main())
