"""The front end the evaluation commands share (evalcli.py), without a GPU: the common options read the same in every command that has
them, the common refusals hold in each, the --compare picture loader's refusals, and what every command's main hands the run opener."""
import importlib

import numpy as np
import pytest
import torch

# command: (argv that makes a sampling run, has --compare and --classes)
COMMANDS = {
    "modes": (["--checkpoint", "c.pt", "--train", "t.npz", "--out", "o"], False),
    "diversity": (["--checkpoint", "c.pt", "--out", "o"], True),
    "swd": (["--checkpoint", "c.pt", "--train", "t.npz", "--out", "o"], True),
    "spectrum": (["--checkpoint", "c.pt", "--train", "t.npz", "--out", "o"], True),
}
WITH_CLASSES = [name for name, (_, full) in COMMANDS.items() if full]
NUM_DEFAULT = {"modes": 10000, "diversity": 2000, "swd": 8192, "spectrum": 8192}


def parse(name, argv):
    return importlib.import_module(name).get_arg_parse(argv)


def test_common_options_read_the_same_in_every_command():
    tail = ["--seed", "5", "--which", "ema", "-b", "8", "--truncation", "0.7", "--prec", "f32", "-m", "CGAN", "--num", "12", "--train", "u.npz"]
    want = {"seed": 5, "which": "ema", "batch_size": 8, "truncation": 0.7, "prec": "f32", "model": "CGAN", "num": 12, "train": "u.npz",
            "checkpoint": "c.pt", "out": "o"}
    for name, (base, full) in COMMANDS.items():
        got = vars(parse(name, base + tail))
        assert {k: got[k] for k in want} == want, name
        assert ("compare" in got, "classes" in got) == (full, full), name
        assert not {"mode", "score", "select", "refine"} & set(got) and ("space" in got) == (name == "modes"), name
        rest = vars(parse(name, base))
        assert (rest["seed"], rest["which"], rest["batch_size"], rest["truncation"], rest["prec"], rest["model"]) == (0, "auto", 64, None, "bf16", "DCGAN"), name
        assert rest["num"] == NUM_DEFAULT[name], name
    for name in WITH_CLASSES:
        a = parse(name, COMMANDS[name][0] + ["-m", "CGAN", "--train", "t.npz", "--classes", "3,17,42"])
        assert a.classes == [3, 17, 42] and a.compare is None, name
        a = parse(name, ["--compare", "a.npz:recon", "dir.x/b.npz", "--out", "o"])
        assert a.compare == [("a.npz", "recon"), ("dir.x/b.npz", "images")], name


@pytest.mark.parametrize("name", sorted(COMMANDS))
def test_common_refusals_hold_in_every_command(name, capsys):
    base, full = COMMANDS[name]
    parse(name, base)
    bad = [["--truncation", "0"], ["-b", "0"], ["--which", "x"], ["--prec", "f16"], ["--num", "-1"]]
    if full:
        bad += [["-m", "CGAN", "--classes", "x"], ["-m", "CGAN", "--classes", "100"], ["-m", "CGAN", "--classes", "-1"], ["-m", "CGAN", "--classes", ""],
                ["--classes", "3"], ["--compare", "a.npz", "b.npz"]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            parse(name, base + extra)
        assert e.value.code == 2, (name, extra)
    if full:
        for argv in (["--compare", "a.npz", "b.npz", "--out", "o", "--train", "t.npz"], ["--compare", "a.npz", "b.npz", "--out", "o", "-m", "CGAN", "--classes", "3"],
                     ["--compare", "a.npz", "--out", "o"], ["--out", "o"]):
            with pytest.raises(SystemExit):
                parse(name, argv)
    capsys.readouterr()


def test_picture_loader_refusals(tmp_path):
    import evalcli
    from hipgan._lib import JckError
    path = str(tmp_path / "p.npz")
    np.savez(path, images=np.zeros((3, 32, 32, 3), np.uint8), f32=np.zeros((3, 32, 32, 3), np.float32),
             wide=np.zeros((3, 32, 64, 3), np.uint8), s48=np.zeros((2, 48, 48, 3), np.uint8), s8=np.zeros((2, 8, 8, 3), np.uint8),
             grey=np.zeros((3, 32, 32, 1), np.uint8), none=np.zeros((0, 32, 32, 3), np.uint8), s160=np.zeros((1, 160, 160, 3), np.uint8))
    sizes = (32, 64, 128)
    x = evalcli.load_u8(path, "images", sizes)
    assert x.dtype == np.uint8 and x.shape == (3, 32, 32, 3) and x.flags["C_CONTIGUOUS"]
    assert evalcli.load_u8(path, "s48", range(11, 129)).shape == (2, 48, 48, 3)
    with pytest.raises(JckError, match=r"no 'nothing' array \(found \["):
        evalcli.load_u8(path, "nothing", sizes)
    for key in ("f32", "wide", "s48", "grey", "none"):
        with pytest.raises(JckError, match=r"must be uint8 \[n,S,S,3\] with S in \(32, 64, 128\), got"):
            evalcli.load_u8(path, key, sizes)
    for key in ("f32", "wide", "s8", "s160", "grey", "none"):
        with pytest.raises(JckError, match=r"must be uint8 \[n,S,S,3\] with 11 <= S <= 128, got"):
            evalcli.load_u8(path, key, range(11, 129))


class Opened(Exception):
    pass


def test_every_command_opens_its_run_the_same_way(tmp_path, monkeypatch):
    """main's head, up to the sampler: a bad training file ends the run before the checkpoint is read; only modes.py --space d demands the
    checkpoint's discriminator, and does so before any engine exists (Sampler.from_checkpoint is stood in for: it needs a GPU)"""
    import evalcli
    from hipgan._lib import JckError
    from hipgan.sampler import Sampler

    def stand_in(cls, ckpt, model, **kw):
        raise Opened(model, kw)
    monkeypatch.setattr(Sampler, "from_checkpoint", classmethod(stand_in))
    labels = np.arange(6) % 3
    np.savez(str(tmp_path / "t.npz"), images=np.zeros((6, 32, 32, 3), np.uint8), labels=labels)
    np.savez(str(tmp_path / "bad.npz"), pictures=np.zeros((6, 32, 32, 3), np.uint8))
    np.savez(str(tmp_path / "bare.npz"), images=np.zeros((6, 32, 32, 3), np.uint8))
    torch.save({"model_g": {"conv1.weight": torch.zeros(1)}}, str(tmp_path / "g.pt"))
    run = lambda train, ckpt="g.pt": ["--checkpoint", str(tmp_path / ckpt), "--train", str(tmp_path / train), "--out", str(tmp_path / "o"), "-b", "8", "--which", "live",
                                       "--prec", "f32"]
    for name in sorted(COMMANDS):
        main = importlib.import_module(name).main
        extra = ["--k", "2"] if name == "modes" else []
        with pytest.raises(JckError, match="bad.npz"):
            main(run("bad.npz", "missing.pt") + extra)                     # the checkpoint does not exist: it was not looked for
        with pytest.raises(JckError, match="has no 'labels' array"):
            main(run("bare.npz", "missing.pt") + extra + ["-m", "CGAN"])
        with pytest.raises(FileNotFoundError):
            main(run("t.npz", "missing.pt") + extra)
        if name == "modes":
            with pytest.raises(JckError, match="model_d"):
                main(run("t.npz") + extra)
            with pytest.raises(JckError, match="--k 7 clusters of the 6 pictures"):
                main(run("bare.npz", "missing.pt") + ["--k", "7", "-m", "CGAN"])
            extra += ["--space", "pixel"]
        with pytest.raises(Opened) as e:
            main(run("t.npz") + extra)
        assert e.value.args == ("DCGAN", {"which": "live", "prec": "f32", "batch": 8, "with_d": False}), name
    # the samples' classes: --classes cycled, else drawn from the training file's labels by the seed; none for a DCGAN, none at --num 0
    a = parse("swd", run("t.npz") + ["-m", "CGAN", "--classes", "3,17", "--num", "5"])
    monkeypatch.setattr(Sampler, "from_checkpoint", classmethod(lambda cls, ckpt, model, **kw: "sampler"))
    s, train_u8, train_labels, cls = evalcli.open_run(a, False)
    assert s == "sampler" and tuple(train_u8.shape) == (6, 32, 32, 3) and train_u8.dtype == torch.uint8 and np.array_equal(np.asarray(train_labels), labels)
    assert cls.tolist() == [3, 17, 3, 17, 3]
    a = parse("swd", run("t.npz") + ["-m", "CGAN", "--num", "5", "--seed", "4"])
    assert evalcli.open_run(a, False)[3].tolist() == labels[np.random.default_rng(5).integers(0, 6, size=5)].tolist()
    assert evalcli.open_run(parse("swd", run("t.npz") + ["--num", "5"]), False)[3] is None
    a = parse("modes", run("bare.npz") + ["-m", "CGAN", "--num", "0", "--labels_out", "p.npz", "--k", "2", "--space", "pixel"])
    assert evalcli.open_run(a, False)[3] is None
    a = parse("diversity", ["--checkpoint", str(tmp_path / "g.pt"), "--out", "o"])
    assert evalcli.open_run(a, False)[1:] == (None, None, None)
