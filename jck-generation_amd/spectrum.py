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

import evalcli


def get_arg_parse(argv=None):
    p = argparse.ArgumentParser(description="power spectra (radial profiles, lattice peaks) of a trained DCGAN / CGAN generator's samples against its "
                                            "training set, or of two picture files", formatter_class=argparse.RawDescriptionHelpFormatter, epilog=__doc__)
    evalcli.add_common_options(p, 8192, "samples, and training pictures they are compared with", train_required=True,
                               compare_help="the pictures of A against those of B",
                               classes_help="CGAN: comma-separated class ids, cycled over the samples; one report per class plus the pooled one")
    p.add_argument("--plane", choices=["luma", "r", "g", "b"], default="luma")
    p.add_argument("--window", choices=["hann"], default=None, help="periodic Hann window in both axes (default: none)")
    return evalcli.check_common(p, p.parse_args(argv), train_required=True)


def settings_of(args):
    return {"plane": args.plane, "window": args.window}


def sheet_of(r):
    """uint8 [3][S][S][3]: the samples' mean spectrum, the training set's, their dB difference"""
    from hipgan.spectrum import render, render_diff
    return np.stack([render(r["mean2d_a"]), render(r["mean2d_b"]), render_diff(r["mean2d_a"], r["mean2d_b"])])


def write(args, r, line):
    from hipgan.spectrum import arrays_of, format_report, to_json
    return evalcli.write_report(args, r, line, "spectrum", to_json, arrays_of, format_report, sheet=(sheet_of(r), 3, "spectrum.png"))


def run_compare(args):
    import torch

    import metrics
    from hipgan._lib import JckError
    from hipgan.spectrum import SIZES
    (pa, ka), (pb, kb) = args.compare
    a, b = evalcli.load_u8(pa, ka, SIZES), evalcli.load_u8(pb, kb, SIZES)
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
    s, train_u8, train_labels, cls = evalcli.open_run(args, False)
    r = s.spectrum(train_u8, n=args.num, seed=args.seed, labels=cls, train_labels=train_labels if args.classes else None, truncation=args.truncation,
                   classes=args.classes, **settings_of(args))
    return write(args, r, f"{r['n']} samples against {r['n']} of {r['n_train']} training pictures")


if __name__ == "__main__":
    sys.exit(main())
