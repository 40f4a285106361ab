"""What a user of the two trainers sees from the host side of an evaluation and of a checkpoint, pinned without a GPU: the
order, arguments and log lines of the best-score ladder (_finish_eval), the files save_model leaves behind, and the order in
which host-RNG mode draws from the CPU generator.  The objects are bare instances (object.__new__) with stand-ins for the
engine, the metric network and the logger."""
import os

import pytest
import torch
import torch.nn as nn

FAMILIES = ["dcgan", "cgan"]
# three evaluations: the first sets every best score; of the other two each criterion improves in exactly one
SCORES = [{"iters": 0, "is": 2.0, "fid": 50.0, "intra": 9.0, "kid": 0.5, "intra_kid": 0.3, "precision": 0.7, "recall": 0.2},
          {"iters": 500, "is": 3.0, "fid": 60.0, "intra": 8.0, "kid": 0.6, "intra_kid": 0.2, "precision": 0.8, "recall": 0.3},
          {"iters": 1000, "is": 2.5, "fid": 40.0, "intra": 8.5, "kid": 0.4, "intra_kid": 0.25, "precision": 0.6, "recall": 0.4}]


def _cls(family):
    if family == "dcgan":
        from train.dcgan_trainer import DCGANTrainer
        return DCGANTrainer
    from train.cgan_trainer import CGANTrainer
    return CGANTrainer


class Log:
    def __init__(self):
        self.lines = []

    def debug(self, msg):
        self.lines.append(msg)

    def warning(self, msg):
        self.lines.append("WARNING " + msg)


class Metric:
    """Hands out SCORES in turn and records which entry point the trainer took."""
    def __init__(self):
        self.calls, self.n = [], -1

    def scores_from_stats(self, logits, stats, splits=10, intra=False):
        self.n += 1
        self.calls.append(("stats", logits, stats, intra))
        s = SCORES[self.n]
        return (s["is"], s["fid"], s["intra"]) if intra else (s["is"], s["fid"])

    def scores_from_logits(self, logits, splits=10, intra=False):
        self.n += 1
        self.calls.append(("logits", logits, None, intra))
        s = SCORES[self.n]
        return (s["is"], s["fid"], s["intra"]) if intra else (s["is"], s["fid"])

    def extra_scores_from_stats(self, stats, intra=False):
        self.calls.append(("extra", None, stats, intra))
        s = SCORES[self.n]
        return {k: s[k] for k in ("kid", "precision", "recall") + (("intra_kid",) if intra else ())}


class Eval:
    def __init__(self, pending):
        self.pending, self.waits = list(pending), []

    def take(self, wait):
        self.waits.append(wait)
        return self.pending.pop(0) if self.pending else None


def _ladder_trainer(family, rank, pending):
    tr = object.__new__(_cls(family))
    tr.rank, tr.metric, tr.logger, tr._eval, tr._image_save_path = rank, Metric(), Log(), Eval(pending), "IMG_DIR"
    tr.saved, tr.pictures = [], []
    tr.save_model = lambda *a: tr.saved.append(a)
    tr.save_image = lambda *a: tr.pictures.append(a)
    return tr


def _pending(family, n, mu, kid, logits=True):
    host = {("images" if family == "dcgan" else "denorm"): f"pic{n}"}
    if logits:
        host["logits"] = f"logits{n}"
        if mu:
            host["mu"] = host["cov"] = 0
        if kid:
            host["kid_rr"] = 0
    return {"iters": SCORES[n]["iters"], "host": host, "snapshot": f"snap{n}"}


def _best0(family):
    return {"fid": 1e10, "is": 0} if family == "dcgan" else {"fid": 1e10, "intra": 1e10, "is": 0}


@pytest.mark.parametrize("kid", [False, True])
@pytest.mark.parametrize("mu", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
def test_finish_eval_ladder(family, mu, kid):
    cgan = family == "cgan"
    pending = [_pending(family, n, mu, kid) for n in range(3)]
    hosts = [p["host"] for p in pending]
    tr = _ladder_trainer(family, 0, pending)
    best = _best0(family)
    for wait in (False, True, True, False):         # the fourth finds nothing pending
        tr._finish_eval(best, wait=wait)
    assert tr._eval.waits == [False, True, True, False]

    # which criterion saves at which evaluation, in the order the ladder tests them
    if cgan:
        improved = [["fid", "intra_fid", "is"] + (["kid", "intra_kid"] if kid else []),
                    ["intra_fid", "is"] + (["intra_kid"] if kid else []),
                    ["fid"] + (["kid"] if kid else [])]
    else:
        improved = [["fid", "is"] + (["kid"] if kid else []), ["is"], ["fid"] + (["kid"] if kid else [])]
    value_of = {"fid": "fid", "is": "is", "kid": "kid"}
    want = []
    for n, typs in enumerate(improved):
        s = SCORES[n]
        for typ in typs:
            if cgan:
                want.append((typ, s["iters"], s["is"], s["fid"], s["intra"], f"pic{n}", f"snap{n}"))
            else:
                want.append((typ, s["iters"], s[value_of[typ]], f"pic{n}", f"snap{n}"))
    assert tr.saved == want

    word = {"fid": "lowest fid", "intra_fid": "lowest intra fid", "is": "highest is", "kid": "lowest kid", "intra_kid": "lowest intra kid"}
    lines = []
    for n, typs in enumerate(improved):
        s = SCORES[n]
        lines.append(f"inception score: {s['is']}\tfid: {s['fid']}" + (f"\tintra fid: {s['intra']}" if cgan else ""))
        if kid:
            lines.append(f"kid: {s['kid']}\tprecision: {s['precision']}\trecall: {s['recall']}"
                         + (f"\tintra kid: {s['intra_kid']}" if cgan else ""))
        lines += [f"{s['iters']} {word[typ]}" for typ in typs]
    assert tr.logger.lines == lines
    assert lines[0] == ("inception score: 2.0\tfid: 50.0\tintra fid: 9.0" if cgan else "inception score: 2.0\tfid: 50.0")
    if kid and cgan:
        assert lines[1] == "kid: 0.5\tprecision: 0.7\trecall: 0.2\tintra kid: 0.3" and "500 lowest intra fid" in lines

    # the device statistics are used when they came back, else the logits alone; the extra scores only from their sums
    calls = [c for c in tr.metric.calls if c[0] != "extra"]
    assert calls == [("stats" if mu else "logits", f"logits{n}", hosts[n] if mu else None, cgan) for n in range(3)]
    assert [c for c in tr.metric.calls if c[0] == "extra"] == ([("extra", None, hosts[n], cgan) for n in range(3)] if kid else [])

    want_best = {"fid": 40.0, "is": 3.0}
    if cgan:
        want_best["intra"] = 8.0
    if kid:
        want_best["kid"] = 0.4
        if cgan:
            want_best["intra_kid"] = 0.2
    assert best == want_best
    assert tr.pictures == ([("IMG_DIR", SCORES[n]["iters"], f"pic{n}") for n in range(3)] if cgan else [])


@pytest.mark.parametrize("family", FAMILIES)
def test_finish_eval_without_a_metric_network_saves_latest(family):
    tr = _ladder_trainer(family, 0, [_pending(family, 1, False, False, logits=False)])
    best = _best0(family)
    tr._finish_eval(best, wait=True)
    if family == "dcgan":
        assert tr.saved == [("latest", 500, 0.0, "pic1", "snap1")] and tr.pictures == []
    else:
        assert tr.saved == [("latest", 500, 0.0, 0.0, 0.0, "pic1", "snap1")] and tr.pictures == [("IMG_DIR", 500, "pic1")]
    assert tr.logger.lines == [] and tr.metric.calls == [] and best == _best0(family)


@pytest.mark.parametrize("logits", [False, True])
def test_cgan_class_grid_is_rank_zeros(logits):
    """save_image after every evaluation on rank 0, never on another rank (save_model has its own rank check)."""
    runs = {}
    for rank in (0, 1):
        tr = _ladder_trainer("cgan", rank, [_pending("cgan", n, True, True, logits=logits) for n in range(3)])
        best = _best0("cgan")
        for _ in range(3):
            tr._finish_eval(best, wait=True)
        runs[rank] = tr
    assert runs[0].pictures == [("IMG_DIR", SCORES[n]["iters"], f"pic{n}") for n in range(3)] and runs[1].pictures == []
    assert runs[1].saved == runs[0].saved and len(runs[0].saved) == (10 if logits else 3)


# ---- save_model --------------------------------------------------------------------------------------------------------------
class Engine:
    def __init__(self, order, ema_decay):
        self.order, self.ema_decay = order, ema_decay

    def join(self):
        self.order.append("join")

    def check(self):
        self.order.append("check")

    def ema_state_dict(self):
        self.order.append("ema")
        return {"weight": torch.full((3, 2), 7.0)}


class Opt:
    def __init__(self, name):
        self.name = name

    def state_dict(self):
        return {"state": {}, "param_groups": [{"name": self.name}]}


FOUR = ["model_d", "model_g", "optimizer_d", "optimizer_g"]


def _saving_trainer(family, tmp_path, monkeypatch, rank=0, ema_decay=None):
    import importlib
    mod = importlib.import_module(f"train.{family}_trainer")
    tr = object.__new__(_cls(family))
    tr.order, tr.pictures = [], []
    tr.rank, tr.model_save_path, tr.logger, tr.engine = rank, str(tmp_path), Log(), Engine(tr.order, ema_decay)
    tr.model_g, tr.model_d = nn.Linear(2, 3), nn.Linear(3, 1)
    tr.optimizer_g, tr.optimizer_d = Opt("g"), Opt("d")
    real_save = torch.save

    def save(obj, path):
        tr.order.append("save")
        real_save(obj, path)
    monkeypatch.setattr(torch, "save", save)
    if family == "dcgan":       # the picture itself is cosmetic (matplotlib); where it goes is not
        monkeypatch.setattr(mod, "_save_png", lambda path, chw, title=None: tr.pictures.append((path, tuple(chw.shape), title)))
    else:
        tr.save_image = lambda path, iters, images: tr.pictures.append((path, iters, images))
    return tr


def _save(tr, family, typ, images, snapshot=None):
    if family == "dcgan":
        tr.save_model(typ, 7, 1.23456, images, snapshot)
        return "7_1.2346.pt"
    tr.save_model(typ, 7, 1.23456, 2.5, 0.12345, images, snapshot)
    return "7_1.2346_2.5000_0.1235.pt"


@pytest.mark.parametrize("ema_decay", [None, 0.999])
@pytest.mark.parametrize("family", FAMILIES)
def test_save_model_live_state(family, ema_decay, tmp_path, monkeypatch):
    tr = _saving_trainer(family, tmp_path, monkeypatch, ema_decay=ema_decay)
    folder = tmp_path / "fid"
    (folder / "dir.pt").mkdir(parents=True)
    (folder / "3_9.0000.pt").write_bytes(b"old")
    (folder / "3_fake_image.png").write_bytes(b"png")
    images = torch.zeros(4, 3, 8, 8)
    name = _save(tr, family, "fid", images)
    assert sorted(os.listdir(folder)) == sorted(["dir.pt", "3_fake_image.png", name])     # the older checkpoint is gone, nothing else
    ck = torch.load(folder / name, weights_only=False)
    assert sorted(ck) == sorted(FOUR + (["model_g_ema"] if ema_decay else []))
    for key, module in (("model_g", tr.model_g), ("model_d", tr.model_d)):
        assert list(ck[key]) == ["weight", "bias"] and all(torch.equal(ck[key][k], v) for k, v in module.state_dict().items())
    assert ck["optimizer_g"]["param_groups"] == [{"name": "g"}] and ck["optimizer_d"]["param_groups"] == [{"name": "d"}]
    if ema_decay:
        assert torch.equal(ck["model_g_ema"]["weight"], torch.full((3, 2), 7.0))
    # the engine is joined first and checked before anything is written
    assert tr.order == ["join"] + (["ema"] if ema_decay else []) + ["check", "save"]
    if family == "dcgan":
        assert tr.pictures == [(str(folder / "7_fake_image.png"), (3, 12, 42), "fake images")] and tr.logger.lines == ["7 model save"]
    else:
        assert len(tr.pictures) == 1 and tr.pictures[0][:2] == (str(folder), 7) and tr.pictures[0][2] is images and tr.logger.lines == []


@pytest.mark.parametrize("family", FAMILIES)
def test_save_model_writes_a_given_snapshot(family, tmp_path, monkeypatch):
    tr = _saving_trainer(family, tmp_path, monkeypatch, ema_decay=0.999)
    snap = {"model_g": {"weight": torch.full((3, 2), 1.0)}, "model_d": {"weight": torch.full((1, 3), 2.0)},
            "optimizer_g": {"snap": "g"}, "optimizer_d": {"snap": "d"}, "model_g_ema": {"weight": torch.full((3, 2), 3.0)},
            "not_a_checkpoint_key": 1}
    name = _save(tr, family, "is", torch.zeros(4, 3, 8, 8), snap)
    ck = torch.load(tmp_path / "is" / name, weights_only=False)
    assert sorted(ck) == sorted(FOUR + ["model_g_ema"])             # snapshot_to_cpu's keys: the stray one is not carried over
    assert float(ck["model_g"]["weight"][0, 0]) == 1.0 and float(ck["model_d"]["weight"][0, 0]) == 2.0
    assert float(ck["model_g_ema"]["weight"][0, 0]) == 3.0 and ck["optimizer_g"] == {"snap": "g"} and ck["optimizer_d"] == {"snap": "d"}
    assert tr.order == ["join", "check", "save"]                    # the live average is not read
    del snap["model_g_ema"]
    name = _save(tr, family, "kid", torch.zeros(4, 3, 8, 8), snap)
    assert sorted(torch.load(tmp_path / "kid" / name, weights_only=False)) == FOUR


@pytest.mark.parametrize("family", FAMILIES)
def test_save_model_is_rank_zeros(family, tmp_path, monkeypatch):
    tr = _saving_trainer(family, tmp_path, monkeypatch, rank=1, ema_decay=0.999)
    _save(tr, family, "fid", torch.zeros(4, 3, 8, 8))
    assert os.listdir(tmp_path) == [] and tr.order == [] and tr.pictures == [] and tr.logger.lines == []


# ---- host-RNG mode: the CPU generator is consumed in the reference's order ---------------------------------------------------
def test_dcgan_host_noise_draw_order():
    tr = object.__new__(_cls("dcgan"))
    tr.host_gen = torch.Generator().manual_seed(7)
    noise = tr._host_noise(2, None)
    g = torch.Generator().manual_seed(7)
    want = {}
    want["n1"] = torch.randn(2, 3, 64, 64, generator=g)
    want["z"] = torch.randn(2, 100, 1, 1, generator=g)
    want["n2"] = torch.randn(2, 3, 64, 64, generator=g)
    want["alpha"] = torch.rand(2, 1, 1, 1, generator=g)
    assert set(noise) == set(want) and all(torch.equal(noise[k], want[k]) for k in want)


def test_cgan_host_noise_draw_order():
    tr = object.__new__(_cls("cgan"))
    tr.host_gen = torch.Generator().manual_seed(7)
    labels = torch.nn.functional.one_hot(torch.tensor([3, 5]), 100)
    noise = tr._host_noise(2, labels)
    g = torch.Generator().manual_seed(7)
    want = {}
    want["n1"] = torch.randn(2, 3, 64, 64, generator=g)
    want["m1"] = torch.empty(2, 256).bernoulli_(0.75, generator=g)
    want["z"] = torch.randn(2, 100, 1, 1, generator=g)
    want["n2"] = torch.randn(2, 3, 64, 64, generator=g)
    want["m2"] = torch.empty(2, 256).bernoulli_(0.75, generator=g)
    want["alpha"] = torch.rand(2, 1, 1, 1, generator=g)
    want["m3"] = torch.empty(2, 256).bernoulli_(0.75, generator=g)
    want["m4"] = torch.empty(2, 256).bernoulli_(0.75, generator=g)
    assert set(noise) == set(want) | {"labels"} and all(torch.equal(noise[k], want[k]) for k in want)
    assert noise["labels"] is labels
