"""Sample diversity of a trained generator from the structural similarity of random pairs, and SSIM / PSNR of two picture files.  Run
from this directory:

    python diversity.py -m CGAN --checkpoint best.pt --num 200 --classes 3,17,42 --pairs 1000 --train train.npz --out diversity
    python diversity.py -m DCGAN --checkpoint best.pt --num 2000 --pairs 1000 --train train.npz --out diversity
    python diversity.py --compare recon/images.npz:images targets.npz --out cmp

--num images are drawn (--truncation, --which, -b as in generate.py; BatchNorm on the running statistics), --pairs random pairs of them
(per class for a CGAN: --classes cycled over the samples, else every sample's class drawn from the training file's `labels` by the seed,
as modes.py does) go through the SSIM / MS-SSIM pair kernel (metrics.ssim_pairs; --levels, default by the networks' size: 64 -> 3,
128 -> 4), and with --train (an .npz with a uint8 `images` array, the networks' size or 32x32 data; `labels` for a CGAN) the training
pictures of each class get the same treatment.  A class whose samples are more similar to each other than its training pictures are -
mean MS-SSIM of the samples above that of the training pictures - is flagged as less diverse (Odena et al. 2017, section 4.3).  Written
to --out:

    diversity.json   levels, n, pairs, samples / train: mean, sem and n of ms_ssim and ssim, overall and per class; share_less_diverse
                     (over the classes both have) and flagged (their ids) when there is a training file; dropped (classes with one sample)
    diversity.npz    i, j (the pairs), group (their class; 0 for a DCGAN), ssim, ms_ssim, sq_err, top (pair indices), and train_* likewise
    diversity.png    the --top sample pairs with the highest MS-SSIM side by side, four pairs a row: near-duplicate samples

and one line: diversity: MS-SSIM 0.0712 +- 0.0011 over 1000 pairs (train 0.0655), 2 of 3 classes less diverse than the training set
--compare A.npz[:key] B.npz[:key] needs no checkpoint: row i of one array against row i of the other (key `images` by default; uint8
[n,S,S,3] of one shape, 11 <= S <= 128) -> compare.npz (psnr, ssim, ms_ssim, sq_err per row) and compare.json (their means): how a
reconstruction from generate.py --project / --inpaint is scored against its input.  On the GPU when there is one, else in numpy."""
import argparse
import sys

import numpy as np
import torch

PAIRS_A_ROW = 4
COMPARE_CHUNK = 4096


def split_key(spec):
    """'file.npz:key' -> (file.npz, key); the key is `images` when none is given"""
    path, sep, key = spec.rpartition(":")
    if sep and path and key and not key.endswith(".npz") and "/" not in key and "\\" not in key:
        return path, key
    return spec, "images"


def get_arg_parse(argv=None):
    p = argparse.ArgumentParser(description="sample diversity (MS-SSIM of random pairs) of a trained DCGAN / CGAN generator; SSIM / PSNR of two files",
                                formatter_class=argparse.RawDescriptionHelpFormatter, epilog=__doc__)
    p.add_argument("-m", "--model", choices=["DCGAN", "CGAN"], default="DCGAN")
    p.add_argument("--checkpoint", default=None, help="a checkpoint written by the trainers (or the reference's)")
    p.add_argument("--compare", nargs=2, default=None, metavar=("A.npz[:key]", "B.npz[:key]"), help="score row i of A against row i of B")
    p.add_argument("--train", default=None, metavar="TRAIN.npz", help="the training pictures: uint8 `images` [N,S,S,3] (and `labels`)")
    p.add_argument("--num", type=int, default=2000, help="samples")
    p.add_argument("--pairs", type=int, default=1000, help="random pairs (per class)")
    p.add_argument("--classes", default=None, help="CGAN: comma-separated class ids, cycled over the samples")
    p.add_argument("--levels", type=int, default=None, help="MS-SSIM levels, 1..4 (default: by the picture size)")
    p.add_argument("--top", type=int, default=16, help="most similar pairs on the sheet")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--which", choices=["auto", "live", "ema"], default="auto")
    p.add_argument("-b", "--batch_size", type=int, default=64, help="images per launch sequence")
    p.add_argument("--truncation", type=float, default=None, help="draw z from a normal truncated to [-T, T]")
    p.add_argument("--prec", choices=["bf16", "f32", "bf16x3"], default="bf16")
    a = p.parse_args(argv)
    if a.levels is not None and not 1 <= a.levels <= 4:
        p.error("--levels must lie in 1..4")
    if a.compare:
        if a.checkpoint or a.train or a.classes:
            p.error("--compare scores two files: --checkpoint, --train and --classes do not go with it")
        a.compare = [split_key(s) for s in a.compare]
        return a
    if not a.checkpoint:
        p.error("--checkpoint is required (or --compare A.npz B.npz)")
    if a.num < 2 or a.pairs < 1 or a.top < 0 or a.batch_size < 1:
        p.error("--num must be >= 2, --pairs >= 1, --top >= 0, -b >= 1")
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
    elif a.model == "CGAN" and not a.train:
        p.error("a CGAN's samples take their classes from --classes or from the `labels` of --train")
    # to generate.check_checkpoint this is a plain sampling run without a discriminator
    a.mode, a.score, a.select, a.refine, a.space = "sample", False, None, None, None
    return a


def load_u8(path, key):
    from hipgan._lib import JckError
    with np.load(path) as f:
        if key not in f.files:
            raise JckError(f"{path}: no '{key}' array (found {sorted(f.files)})")
        x = f[key]
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2] or x.shape[0] < 1 or not 11 <= x.shape[1] <= 128:
        raise JckError(f"{path}: '{key}' must be uint8 [n,S,S,3] with 11 <= S <= 128, got {x.dtype} {tuple(x.shape)}")
    return np.ascontiguousarray(x)


def run_compare(args):
    import metrics
    from generate import write_outputs
    from hipgan._lib import JckError
    (pa, ka), (pb, kb) = args.compare
    a, b = load_u8(pa, ka), load_u8(pb, kb)
    if a.shape != b.shape:
        raise JckError(f"--compare: {pa} holds {a.shape}, {pb} holds {b.shape}")
    on_dev = torch.cuda.is_available()
    parts = []
    for lo in range(0, a.shape[0], COMPARE_CHUNK):
        xa, xb = a[lo:lo + COMPARE_CHUNK], b[lo:lo + COMPARE_CHUNK]
        if on_dev:
            xa, xb = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
        idx = np.arange(xa.shape[0], dtype=np.int64)
        parts.append({k: metrics._host(v) for k, v in metrics.ssim_pairs(xa, xb, idx, idx, levels=args.levels).items()})
    arrays = {k: np.concatenate([p[k] for p in parts]) for k in ("ssim", "ms_ssim", "sq_err")}
    arrays["psnr"] = metrics.psnr(arrays["sq_err"], a.shape[1])
    record = {"n": int(a.shape[0]), "size": int(a.shape[1]), **{k: float(np.mean(arrays[k].astype(np.float64))) for k in ("psnr", "ssim", "ms_ssim", "sq_err")}}
    write_outputs(args.out, "compare.npz", arrays, record=("compare.json", record))
    print(f"compare: {a.shape[0]} pictures, PSNR {record['psnr']:.2f} dB, SSIM {record['ssim']:.4f}, MS-SSIM {record['ms_ssim']:.4f} "
          f"-> {args.out}/compare.json, compare.npz")
    return 0


def side_of(summary):
    """the JSON form of {"ms_ssim", "ssim": summarise()}: mean / sem / n overall and per class"""
    cut = lambda s: {"mean": s["mean"], "sem": s["sem"], "n": s["n"]}
    return {key: {**cut(s), "per_class": {str(c): cut(v) for c, v in s["per_class"].items()}} for key, s in summary.items()}


def main(argv=None):
    args = get_arg_parse(argv)
    if args.compare:
        return run_compare(args)
    from generate import check_checkpoint, write_outputs
    from hipgan.probe import load_images
    from hipgan.sampler import Sampler
    from modes import sample_classes
    train_u8, train_labels = load_images(args.train) if args.train else (None, None)      # a bad file ends the run before a checkpoint is read
    if args.classes:
        cls = torch.tensor([args.classes[k % len(args.classes)] for k in range(args.num)])
    else:
        cls = sample_classes(args, train_labels, args.num)
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    check_checkpoint(args, ckpt)
    s = Sampler.from_checkpoint(ckpt, args.model, which=args.which, prec=args.prec, batch=args.batch_size)
    r = s.diversity(args.num, pairs=args.pairs, seed=args.seed, labels=cls, train_u8=train_u8, train_labels=train_labels, levels=args.levels,
                    truncation=args.truncation, top=args.top)
    group = lambda pr: pr["group"] if pr["group"] is not None else np.zeros(pr["i"].shape[0], np.int64)
    arrays = {"i": r["pairs"]["i"], "j": r["pairs"]["j"], "group": group(r["pairs"]), "ssim": r["ssim"], "ms_ssim": r["ms_ssim"],
              "sq_err": r["sq_err"], "top": r["top"]}
    record = {"levels": r["levels"], "n": args.num, "pairs": args.pairs, "samples": side_of(r["summary"]), "train": None,
              "share_less_diverse": None, "flagged": [], "dropped": [int(c) for c in r["dropped"]]}
    ms = r["summary"]["ms_ssim"]
    tail = ""
    if "train" in r:
        t, c = r["train"], r["comparison"]
        arrays.update({"train_i": t["pairs"]["i"], "train_j": t["pairs"]["j"], "train_group": group(t["pairs"]), "train_ssim": t["ssim"],
                       "train_ms_ssim": t["ms_ssim"], "train_sq_err": t["sq_err"]})
        record.update(train=side_of(t["summary"]), share_less_diverse=c["share_less_diverse"], flagged=[int(k) for k in c["flagged"]])
        tail = (f" (train {t['summary']['ms_ssim']['mean']:.4f}), {len(c['flagged'])} of {len(c['per_class'])} classes less diverse than the "
                f"training set")
    images = r["images"].cpu().numpy()
    at = np.stack([r["pairs"]["i"][r["top"]], r["pairs"]["j"][r["top"]]], axis=1).reshape(-1)
    sheet = (images[at], 2 * PAIRS_A_ROW, "diversity.png") if at.size else None
    write_outputs(args.out, "diversity.npz", arrays, sheet=sheet, record=("diversity.json", record))
    print(f"diversity: MS-SSIM {ms['mean']:.4f} +- {ms['sem']:.4f} over {ms['n']} pairs{tail} -> {args.out}/diversity.json, diversity.npz"
          + (", diversity.png" if sheet else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
