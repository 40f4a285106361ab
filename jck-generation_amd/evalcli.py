"""What the evaluation commands (modes.py, diversity.py, swd.py, spectrum.py) share: the options every one of them takes and the checks
that follow parsing, the picture-file loader of --compare, the opening of a run on a checkpoint and a training file, and the report
writer of the commands that compare samples with the training set.  Host only; torch is imported where a run needs it."""
import numpy as np

TRAIN_HELP = "the training pictures: uint8 `images` [N,S,S,3] (and `labels`)"


def add_common_options(p, num, num_help, train_help=TRAIN_HELP, train_required=False, compare_help=None, classes_help=None):
    """-m, --checkpoint, --train, --num, --out, --seed, --which, -b, --truncation, --prec and, where the command gives their help
    strings, --compare and --classes.  A command without --compare has argparse demand --checkpoint (and --train, with train_required);
    one with it leaves that to check_common."""
    from generate import parse_classes
    must = compare_help is None
    p.add_argument("-m", "--model", choices=["DCGAN", "CGAN"], default="DCGAN")
    p.add_argument("--checkpoint", default=None, required=must, help="a checkpoint written by the trainers (or the reference's)")
    if compare_help:
        p.add_argument("--compare", nargs=2, default=None, metavar=("A.npz[:key]", "B.npz[:key]"), help=compare_help)
    p.add_argument("--train", default=None, required=must and train_required, metavar="TRAIN.npz", help=train_help)
    p.add_argument("--num", type=int, default=num, help=num_help)
    if classes_help:
        p.add_argument("--classes", type=parse_classes, default=None, help=classes_help)
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--which", choices=["auto", "live", "ema"], default="auto")
    p.add_argument("-b", "--batch_size", type=int, default=64, help="images per launch sequence")
    p.add_argument("--truncation", type=float, default=None, help="draw z from a normal truncated to [-T, T]")
    p.add_argument("--prec", choices=["bf16", "f32", "bf16x3"], default="bf16")


def check_common(p, a, train_required=False, num_min=1):
    """The checks on the common options, after parse_args.  With --compare the two file arguments become (path, key) pairs and nothing
    else is looked at: the options of a sampling run do not go with it."""
    if getattr(a, "compare", None):
        if a.checkpoint or a.train or a.classes:
            p.error("--compare takes two files: --checkpoint, --train and --classes do not go with it")
        a.compare = [split_key(s) for s in a.compare]
        return a
    if not a.checkpoint or (train_required and not a.train):
        p.error(("--checkpoint and --train are" if train_required else "--checkpoint is") + " required (or --compare A.npz B.npz)")
    if a.num < num_min or a.batch_size < 1:
        p.error(f"--num must be >= {num_min}, -b >= 1")
    if a.truncation is not None and not a.truncation > 0:
        p.error("--truncation must be > 0")
    if getattr(a, "classes", None) is not None and a.model != "CGAN":
        p.error("--classes goes with -m CGAN")
    return a


def split_key(spec):
    """'file.npz:key' -> (file.npz, key); the key is `images` when none is given"""
    path, sep, key = spec.rpartition(":")
    if sep and path and key and not key.endswith(".npz") and "/" not in key and "\\" not in key:
        return path, key
    return spec, "images"


def load_u8(path, key, sizes):
    """The uint8 [n,S,S,3] array `key` of the .npz at `path`, contiguous; sizes: the S a command takes, a collection or a range"""
    from hipgan._lib import JckError
    with np.load(path) as f:
        if key not in f.files:
            raise JckError(f"{path}: no '{key}' array (found {sorted(f.files)})")
        x = f[key]
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2] or x.shape[0] < 1 or x.shape[1] not in sizes:
        want = f"{sizes[0]} <= S <= {sizes[-1]}" if isinstance(sizes, range) else f"S in {sizes}"
        raise JckError(f"{path}: '{key}' must be uint8 [n,S,S,3] with {want}, got {x.dtype} {tuple(x.shape)}")
    return np.ascontiguousarray(x)


def sample_classes(args, train_labels, n):
    """class ids [n] of a CGAN's samples (None for a DCGAN): drawn with the seed from the training file's labels"""
    import torch
    from hipgan._lib import JckError
    if args.model != "CGAN":
        return None
    if train_labels is None:
        raise JckError(f"{args.train} has no 'labels' array: a CGAN's samples take their classes from it")
    if train_labels.min() < 0 or train_labels.max() > 99:
        raise JckError(f"{args.train}: 'labels' must lie in 0..99")
    return torch.as_tensor(train_labels[np.random.default_rng(args.seed + 1).integers(0, train_labels.shape[0], size=n)])


def open_run(args, with_d, check_train=None):
    """(sampler, training pictures, training labels, class ids of the --num samples) of a run on --checkpoint: the training file is read
    first (a bad one, or one check_train(pictures) refuses, ends the run before a checkpoint is read), then the samples' classes are
    settled (--classes cycled, else a CGAN's drawn from the file's labels), then the checkpoint is read and, with_d, its discriminator
    demanded before any engine exists."""
    import torch
    from hipgan.probe import load_images
    from hipgan.sampler import Sampler, pick_discriminator_state
    train_u8, train_labels = load_images(args.train) if args.train else (None, None)
    if check_train:
        check_train(train_u8)
    classes = getattr(args, "classes", None)
    if classes:
        cls = torch.tensor([classes[k % len(classes)] for k in range(args.num)])
    else:
        cls = sample_classes(args, train_labels, args.num) if args.num else None
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    if with_d:
        pick_discriminator_state(ckpt)
    s = Sampler.from_checkpoint(ckpt, args.model, which=args.which, prec=args.prec, batch=args.batch_size, with_d=bool(with_d))
    return s, train_u8, train_labels, cls


def write_report(args, r, line, stem, to_json, arrays_of, format_report, extra=None, sheet=None):
    """<stem>.json, <stem>.npz (and the sheet) of a samples-against-training-set report r in --out, and the command's one line:
    to_json(r) and `extra` make the record, arrays_of(r, suffix) the arrays; with r["per_class"] the record gets the same per class id
    and the arrays once more with the suffix _<class id>."""
    from generate import write_outputs
    record = {**to_json(r), **(extra or {})}
    arrays = arrays_of(r, "")
    if "per_class" in r:
        record["per_class"] = {str(c): to_json(v) for c, v in r["per_class"].items()}
        for c, v in r["per_class"].items():
            arrays.update(arrays_of(v, f"_{c}"))
    write_outputs(args.out, f"{stem}.npz", arrays, sheet=sheet, record=(f"{stem}.json", record))
    files = [f"{args.out}/{stem}.json", f"{stem}.npz"] + ([sheet[2]] if sheet else [])
    print(f"{stem}: {format_report(r)} ({line}) -> {', '.join(files)}")
    return 0
