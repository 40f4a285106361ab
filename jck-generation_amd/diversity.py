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

from evalcli import add_common_options, check_common, load_u8, open_run, split_key  # noqa: F401  (split_key: part of this module's interface)

PAIRS_A_ROW = 4
COMPARE_CHUNK = 4096


def get_arg_parse(argv=None):
    p = argparse.ArgumentParser(description="sample diversity (MS-SSIM of random pairs) of a trained DCGAN / CGAN generator; SSIM / PSNR of two files",
                                formatter_class=argparse.RawDescriptionHelpFormatter, epilog=__doc__)
    add_common_options(p, 2000, "samples", compare_help="score row i of A against row i of B",
                       classes_help="CGAN: comma-separated class ids, cycled over the samples")
    p.add_argument("--pairs", type=int, default=1000, help="random pairs (per class)")
    p.add_argument("--levels", type=int, default=None, help="MS-SSIM levels, 1..4 (default: by the picture size)")
    p.add_argument("--top", type=int, default=16, help="most similar pairs on the sheet")
    a = p.parse_args(argv)
    if a.levels is not None and not 1 <= a.levels <= 4:
        p.error("--levels must lie in 1..4")
    check_common(p, a, num_min=2)
    if a.compare:
        return a
    if a.pairs < 1 or a.top < 0:
        p.error("--pairs must be >= 1, --top >= 0")
    if a.classes is None and a.model == "CGAN" and not a.train:
        p.error("a CGAN's samples take their classes from --classes or from the `labels` of --train")
    return a


def run_compare(args):
    import metrics
    from generate import write_outputs
    from hipgan._lib import JckError
    (pa, ka), (pb, kb) = args.compare
    a, b = load_u8(pa, ka, range(11, 129)), load_u8(pb, kb, range(11, 129))
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
    from generate import write_outputs
    s, train_u8, train_labels, cls = open_run(args, False)
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
