"""The samples-against-training-set driver of Sampler (swd, spectrum) and the commands on it, on the GPU, to the bit: the pooled spectrum
report rebuilt by hand, as test_swd_gpu does for swd; spectrum.main on the tiny trained checkpoint; the --classes path through swd.main
and spectrum.main against the Sampler methods.  n = 16 at batch 8 is two engine launches; 24 training pictures leave the permutation
something to drop; 12 samples of two classes against 8 training pictures of each leave six a class, the samples' side being the smaller."""
import json
import os

import numpy as np
import pytest
import torch

from test_swd_gpu import cuda, trained  # noqa: F401  (the tiny trained checkpoint and its training file, built once for this module)

pytestmark = pytest.mark.gpu


def same(a, b):
    """bit equality of two report values: arrays and numbers by their bytes, containers item by item"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or isinstance(a, str):
        return a == b
    x, y = np.asarray(a), np.asarray(b)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_sampler_spectrum_is_the_report_of_the_two_sets_built_by_hand(trained):
    import metrics
    from hipgan.sampler import latents
    s, train = trained["sampler"], trained["train"]
    r = s.spectrum(train, n=16, seed=3, window="hann")
    assert (r.pop("n"), r.pop("n_train"), r.pop("seed")) == (16, 24, 3)
    pick = np.random.default_rng(3).permutation(24)[:16]                            # the definition, written out
    kw = dict(window="hann", mean2d=True)
    own = metrics.spectrum_report(metrics.spectrum(s.from_latents(latents(16, 3)), **kw), metrics.spectrum(cuda(train[pick]), **kw))
    arrays = [k for k, v in own.items() if isinstance(v, np.ndarray)]
    assert {"radius", "count", "mean_db_a", "std_db_a", "mean_db_b", "std_db_b", "gap_db", "z", "mean2d_a", "mean2d_b"} <= set(arrays)
    for k in arrays:
        assert same(r[k], own[k]), k
    assert same(r, own)


def test_spectrum_command_line_on_the_trained_checkpoint(trained):
    import spectrum
    from hipgan import spectrum as H
    out = trained["dir"] / "spectrum_out"
    assert spectrum.main(["-m", "DCGAN", "--checkpoint", trained["ckpt"], "--train", str(trained["dir"] / "train.npz"), "--num", "16", "--seed", "3", "-b", "8",
                          "--window", "hann", "--out", str(out)]) == 0
    r = trained["sampler"].spectrum(trained["train"], n=16, seed=3, window="hann")
    rec = json.load(open(str(out / "spectrum.json")))
    assert rec == json.loads(json.dumps(H.to_json(r))) and (rec["n"], rec["n_train"], rec["seed"], rec["window"]) == (16, 24, 3, "hann")
    f, want = np.load(str(out / "spectrum.npz")), H.arrays_of(r)
    assert set(f.files) == set(want) and {"gap_db", "mean2d_a", "mean2d_b"} <= set(want)
    for k, v in want.items():
        assert same(f[k], v), k
    assert os.path.getsize(str(out / "spectrum.png")) > 0


@pytest.fixture(scope="module")
def cgan(tmp_path_factory):
    """the fresh CGAN of the per-class tests as a checkpoint file, and their labelled training file: eight pictures of each of three classes"""
    from hipgan.engine import CganEngine
    from oracle.gan_oracle import GanOracle
    d = tmp_path_factory.mktemp("evalcli")
    orc = GanOracle("cgan", lr=2e-4, seed=12345)
    eng = CganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gs, ds = eng.state_dicts()
    torch.save({"model_g": gs, "model_d": ds}, str(d / "cgan.pt"))
    train, labels = np.random.default_rng(92).integers(0, 256, size=(24, 64, 64, 3), dtype=np.uint8), np.array([3, 17, 42] * 8)
    np.savez(str(d / "train.npz"), images=train, labels=labels)
    return {"dir": d, "ckpt": str(d / "cgan.pt"), "train": train, "labels": labels}


def test_classes_path_through_the_commands(cgan):
    import spectrum
    import swd
    from hipgan import spectrum as H
    from hipgan.sampler import Sampler
    s = Sampler.from_checkpoint(cgan["ckpt"], "CGAN", batch=8)
    common = ["-m", "CGAN", "--checkpoint", cgan["ckpt"], "--train", str(cgan["dir"] / "train.npz"), "--classes", "3,17", "--num", "12", "--seed", "1", "-b", "8"]
    of = dict(n=12, seed=1, labels=torch.tensor([3, 17] * 6), train_labels=cgan["labels"], classes=[3, 17])        # --classes, cycled over the samples
    settings = dict(patches=4, dirs=4, repeats=1)
    r = s.swd(cgan["train"], **of, **settings)
    out = cgan["dir"] / "swd_out"
    assert swd.main(common + ["--patches", "4", "--dirs", "4", "--repeats", "1", "--out", str(out)]) == 0
    rec, f = json.load(open(str(out / "swd.json"))), np.load(str(out / "swd.npz"))
    assert set(rec["per_class"]) == {"3", "17"} and rec["n"] == 12 and rec["settings"] == settings
    assert sorted(f.files) == ["per_repeat", "per_repeat_17", "per_repeat_3"] and same(f["per_repeat"], r["per_repeat"])
    for c in (3, 17):
        assert rec["per_class"][str(c)]["n"] == r["per_class"][c]["n"] == 6
        assert rec["per_class"][str(c)]["swd"] == [float(v) for v in r["per_class"][c]["swd"]]
        assert same(f[f"per_repeat_{c}"], r["per_class"][c]["per_repeat"]), c
    r = s.spectrum(cgan["train"], **of)
    out = cgan["dir"] / "spectrum_out"
    assert spectrum.main(common + ["--out", str(out)]) == 0
    rec, f = json.load(open(str(out / "spectrum.json"))), np.load(str(out / "spectrum.npz"))
    assert set(rec["per_class"]) == {"3", "17"} and rec["n"] == 12
    want = H.arrays_of(r)
    for c in (3, 17):
        assert rec["per_class"][str(c)] == json.loads(json.dumps(H.to_json(r["per_class"][c]))) and rec["per_class"][str(c)]["n"] == r["per_class"][c]["n"] == 6
        want.update(H.arrays_of(r["per_class"][c], f"_{c}"))
    assert set(f.files) == set(want) and {"gap_db_3", "gap_db_17", "mean2d_a_3", "mean2d_b_17"} <= set(want)
    for k, v in want.items():
        assert same(f[k], v), k
    assert os.path.getsize(str(out / "spectrum.png")) > 0
