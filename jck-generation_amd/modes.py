"""Mode coverage of a trained generator: did it collapse, and which modes of the training set are missing?  Run from this directory:

    python modes.py -m DCGAN --checkpoint best.pt --train train.npz --k 100 --num 10000 --out modes
    python modes.py -m DCGAN --checkpoint best.pt --train train.npz --k 100 --num 0 --labels_out pseudo.npz --out modes

The training pictures (--train: an .npz with a uint8 `images` array, the networks' size or 32x32 data, upscaled as the trainers do) are
clustered by k-means on the device (hipgan.cluster.kmeans: k-means++ from --seed, at most --iters updates) in the discriminator's
block-normalised feature space (--space d, the default; --grid, --pool as generate.py --features takes them) or in pixel space
(--space pixel, which needs no discriminator).  --num images are drawn (--truncation, --which, -b as in generate.py; BatchNorm on the
running statistics; a CGAN draws every sample's class from the training file's `labels`, by the seed, so that the class proportions
match), their rows are made the same way and each goes to its nearest centre.  Written to --out:

    modes.json    k, k_real (clusters with a training picture), covered (clusters with at least --min_count samples), expected_covered
                  (what a perfect generator reaches with --num samples), kl = KL(samples || train) of the two histograms in nats,
                  inertia and iters of the clustering, n, space, missing (uncovered cluster ids, largest first, at most 32)
    modes.npz     centres fp32 [k,D], train_labels int64 [N], hist_real / hist_fake int64 [k], sample_cluster int64 [n], sample_d2 fp32 [n]
    modes.png     a row for each of the 16 clusters with the fewest samples for their size: the 8 training pictures nearest the centre,
                  then the 8 samples nearest it (black where there are fewer)

and one line: modes: 87 of 100 clusters covered (expected 99.3 at n = 10000), KL(samples || train) 0.1432
--labels_out FILE.npz writes the training pictures again with `labels` set to their cluster ids - pseudo-labels with which
`main.py -m CGAN --data FILE.npz` trains the conditional model on unlabelled pictures (--k at most 100: its classes are 0..99);
--num 0 then skips the sampling."""
import argparse
import os
import sys

import numpy as np
import torch

import evalcli

SHEET_ROWS, SHEET_SIDE = 16, 8


def get_arg_parse(argv=None):
    p = argparse.ArgumentParser(description="mode coverage of a trained DCGAN / CGAN generator", formatter_class=argparse.RawDescriptionHelpFormatter,
                                epilog=__doc__)
    evalcli.add_common_options(p, 10000, "samples (0 with --labels_out: cluster only)", train_help="the training pictures: uint8 `images` [N,S,S,3]",
                               train_required=True)
    p.add_argument("--k", type=int, default=100, help="clusters, 1..1024")
    p.add_argument("--space", choices=["d", "pixel"], default="d", help="the discriminator's features, or pixels")
    p.add_argument("--grid", type=int, choices=[1, 2, 4], default=4, help="--space d: the pooling raster")
    p.add_argument("--pool", choices=["max", "mean"], default="max", help="--space d")
    p.add_argument("--iters", type=int, default=50, help="Lloyd updates at most")
    p.add_argument("--min_count", type=int, default=1, help="samples a cluster needs to count as covered")
    p.add_argument("--labels_out", default=None, metavar="FILE.npz", help="the training pictures with their cluster ids as `labels`")
    a = p.parse_args(argv)
    if not 1 <= a.k <= 1024:
        p.error("--k must lie in 1..1024")
    if a.labels_out and a.k > 100:
        p.error("--labels_out writes class ids for the CGAN, which takes 0..99: --k must be <= 100")
    if a.num < 0 or (a.num == 0 and not a.labels_out):
        p.error("--num must be >= 1 (0 only with --labels_out: cluster and stop)")
    if a.iters < 0 or a.min_count < 1 or a.batch_size < 1:
        p.error("--iters must be >= 0, --min_count >= 1, -b >= 1")
    return evalcli.check_common(p, a, train_required=True, num_min=0)


def write_labels(path, images_u8, labels):
    """the pictures (uint8 [N,S,S,3]) with int64 `labels` [N]: the file main.py --data takes (load_npz_dataset)"""
    path = path if path.endswith(".npz") else path + ".npz"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, images=np.ascontiguousarray(np.asarray(images_u8), dtype=np.uint8), labels=np.asarray(labels).astype(np.int64).reshape(-1))
    return path


def check_k(args, train_u8):
    from hipgan._lib import JckError
    if args.k > train_u8.shape[0]:
        raise JckError(f"--k {args.k} clusters of the {train_u8.shape[0]} pictures of {args.train}")


def least_covered(r, rows=SHEET_ROWS):
    """the ids of the `rows` clusters with the lowest hist_fake / (n p_c), lowest first (ties: the lower id)"""
    real, fake = r["hist_real"].astype(np.float64), r["hist_fake"].astype(np.float64)
    ids = np.flatnonzero(real > 0)
    ratio = fake[ids] / (max(1.0, fake.sum()) * real[ids] / real.sum())
    return ids[np.argsort(ratio, kind="stable")][:rows]


def nearest_members(cluster_of, d2, c, side=SHEET_SIDE):
    """the `side` members of cluster c nearest its centre, nearest first"""
    members = np.flatnonzero(cluster_of == c)
    return members[np.argsort(d2[members], kind="stable")][:side]


def sheet(s, train_u8, r, cls):
    """uint8 [rows * 16, S,S,3]: per least-covered cluster its 8 nearest training pictures, then its 8 nearest samples"""
    from hipgan.probe import _to_size
    order = least_covered(r)
    size = s.engine.size
    cells = np.zeros((order.shape[0], 2 * SHEET_SIDE, size, size, 3), np.uint8)
    picks = []
    for row, c in enumerate(order):
        tr = nearest_members(r["train_labels"], r["train_d2"], c)
        if tr.size:
            cells[row, :tr.size] = _to_size(train_u8[torch.as_tensor(tr)], size, "training images").cpu().numpy()
        sm = nearest_members(r["sample_cluster"], r["sample_d2"], c)
        picks += [(row, SHEET_SIDE + j, int(i)) for j, i in enumerate(sm)]
    if picks:                             # the pictures of these latents once more: under running statistics each is a function of its own z
        at = torch.as_tensor([i for _, _, i in picks])
        u8 = s.from_latents(torch.as_tensor(r["z"])[at], None if cls is None else cls[at]).cpu().numpy()
        for (row, col, _), pic in zip(picks, u8):
            cells[row, col] = pic
    return cells.reshape((-1,) + cells.shape[2:])


def main(argv=None):
    args = get_arg_parse(argv)
    from generate import write_outputs
    s, train_u8, _, cls = evalcli.open_run(args, args.space == "d", check_train=lambda t: check_k(args, t))
    cl = s.cluster(train_u8, args.k, space=args.space, seed=args.seed, iters=args.iters, grid=args.grid, pool=args.pool)
    if args.labels_out:
        path = write_labels(args.labels_out, train_u8.numpy(), cl["labels"].cpu().numpy())
        print(f"pseudo-labels: {train_u8.shape[0]} pictures in {int((cl['count'] > 0).sum())} clusters -> {path}")
    if not args.num:
        return 0
    r = s.modes(train_u8, n=args.num, seed=args.seed, truncation=args.truncation, labels=cls, clusters=cl, min_count=args.min_count,
                space=args.space, grid=args.grid, pool=args.pool)
    record = {"k": r["k"], "k_real": r["k_real"], "covered": r["covered"], "expected_covered": r["expected_covered"], "kl": r["kl"],
              "inertia": r["inertia"], "iters": r["iters"], "n": args.num, "space": args.space, "missing": [int(c) for c in r["missing"][:32]]}
    arrays = {key: r[key] for key in ("centres", "train_labels", "hist_real", "hist_fake", "sample_cluster", "sample_d2")}
    write_outputs(args.out, "modes.npz", arrays, sheet=(sheet(s, train_u8, r, cls), 2 * SHEET_SIDE, "modes.png"), record=("modes.json", record))
    print(f"modes: {r['covered']} of {r['k_real']} clusters covered (expected {r['expected_covered']:.1f} at n = {args.num}), "
          f"KL(samples || train) {r['kl']:.4f} -> {args.out}/modes.json, modes.npz, modes.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
