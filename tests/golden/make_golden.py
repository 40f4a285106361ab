#!/usr/bin/env python3
"""Golden-vector generator.  RUNS ONLY IN THE BUILD CONTAINER.

Imports the *unmodified* reference (`/root/reference`) under in-memory stubs for the two
third-party packages this image lacks (torchinfo, torchvision) and records what the reference
computes on seeded synthetic inputs.  Only DATA (scalars, checksums, sampled elements) is written
to `tests/golden/*.json`; no reference source travels.  Method: SURVEY.md section 8c.

    python tests/golden/make_golden.py            # regenerates every fixture (about 2 min of CPU)

Fixtures
  modules.json      forward/backward of the four nets on B=4 seeded inputs
  dcgan_steps.json  real DCGANTrainer.train() for 3 steps, B=8 and B=64, lr 2e-4 (+ lr 0.1 clamp run)
  cgan_steps.json   real CGANTrainer.train() for 2 steps, B=8 and B=32, lr 2e-4
  metrics.json      Metrics.inception_score / fid / intra_fid on seeded 100-d features
  selfdiv.json      reference vs itself (8 threads vs 1 thread): long-horizon noise floor

Two fixtures record the project's own GPU results, not the reference's; they need an MI355X and no reference, and are written
only when named:

    python tests/golden/make_golden.py --only latent_plain_bits --commit <the commit the library was built from>
    python tests/golden/make_golden.py --only infer_bits --commit <the commit the library was built from>

  latent_plain_bits.json   SHA-256 of the raw output bytes of the plain latent entry points (jck_latent_loss,
                           jck_engine_latent_grad, jck_engine_project); tests/test_latent_plain_bits_gpu.py recomputes them
  infer_bits.json          the same of the _ex / _fm latent entry points with a weight, a critic and a feature term, of
                           jck_engine_score and jck_engine_features, and of the engine's Python methods over them; every digest is
                           computed twice and written only if the two agree; tests/test_infer_bits_gpu.py recomputes them

Two more record generate.py at a commit, the first on the CPU, the second on an MI355X:

    python tests/golden/make_golden.py --only generate_cli --commit <the commit checked out>
    python tests/golden/make_golden.py --only generate_bits --commit <the commit checked out and built>

  generate_cli.json        which of 8758 command lines the parser refuses, and a digest of the namespace of each it accepts;
                           tests/test_generate_table_cpu.py reproduces it
  generate_bits.json       SHA-256 of every array, .png, .json and printed line of one generate.main run per mode and sampling
                           strategy, each run twice as above; tests/test_generate_bits_gpu.py reproduces it
"""
import argparse
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_SEED = 12345          # change_randomseed.py:1
DATA_SEED = 2024


# --------------------------------------------------------------------------------------------
# stubs for the packages the image lacks (ordinary ModuleNotFoundError otherwise)
# --------------------------------------------------------------------------------------------
def install_stubs():
    import matplotlib
    matplotlib.use("Agg")
    ti = types.ModuleType("torchinfo")
    ti.summary = lambda *a, **k: "<summary stub>"
    sys.modules["torchinfo"] = ti

    tv = types.ModuleType("torchvision")
    tvu = types.ModuleType("torchvision.utils")

    def make_grid(t, padding=2, normalize=False, **k):
        t = t.detach().cpu()
        return t[0] if t.dim() == 4 else t
    tvu.make_grid = make_grid
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")

    def resize(img, size, **k):
        return torch.nn.functional.interpolate(img, size=size, mode="bilinear", align_corners=False)
    tvf.resize = resize
    tvt.functional = tvf
    tvm = types.ModuleType("torchvision.models")
    tvd = types.ModuleType("torchvision.datasets")
    tv.utils, tv.transforms, tv.models, tv.datasets = tvu, tvt, tvm, tvd
    for name, mod in [("torchvision", tv), ("torchvision.utils", tvu), ("torchvision.transforms", tvt),
                      ("torchvision.transforms.functional", tvf), ("torchvision.models", tvm),
                      ("torchvision.datasets", tvd)]:
        sys.modules[name] = mod


# --------------------------------------------------------------------------------------------
# tensor digests
# --------------------------------------------------------------------------------------------
def sample_idx(name, numel, k=8):
    h = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    rng = np.random.default_rng(h)
    return rng.integers(0, numel, size=min(k, numel)).tolist()


def digest(name, t):
    a = t.detach().cpu().double().reshape(-1).numpy()
    idx = sample_idx(name, a.size)
    return {"shape": list(t.shape), "sum": float(a.sum()), "abssum": float(np.abs(a).sum()),
            "l2": float(np.sqrt((a * a).sum())), "idx": idx, "vals": [float(a[i]) for i in idx]}


def digest_dict(prefix, named):
    return {k: digest(prefix + k, v) for k, v in named}


def synth_images(n, seed=DATA_SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, 64, 64, generator=g) * 2 - 1


def synth_onehot(n, seed=DATA_SEED + 1, classes=100):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, classes, (n,), generator=g)
    return torch.nn.functional.one_hot(lab, 100).to(torch.int64), lab


# --------------------------------------------------------------------------------------------
# module-level goldens
# --------------------------------------------------------------------------------------------
def gen_modules():
    from model import DCGAN, CGAN
    out = {}
    B = 4
    for fam, mod in (("dcgan", DCGAN), ("cgan", CGAN)):
        torch.manual_seed(MODEL_SEED)
        g, d = mod.Generator(), mod.Discriminator()
        g.apply(mod.weights_init)
        d.apply(mod.weights_init)
        gen = torch.Generator().manual_seed(77)
        z = torch.randn(B, 100, 1, 1, generator=gen)
        x = synth_images(B, seed=99).requires_grad_(True)
        rg = torch.randn(B, 3, 64, 64, generator=gen)
        rd = torch.randn(B, generator=gen)
        oh, _ = synth_onehot(B, seed=5)
        rec = {"init_g": digest_dict(fam + ".g.", g.state_dict().items()),
               "init_d": digest_dict(fam + ".d.", d.state_dict().items())}
        if fam == "cgan":
            d.drop1.p = 0.0    # dropout mask is RNG-dependent; module golden pins the p=0 function
            fake = g(z, oh)
            dout = d(x, oh).view(-1)
        else:
            fake = g(z)
            dout = d(x).view(-1)
        (fake * rg).sum().backward()
        (dout * rd).sum().backward()
        rec["g_out"] = digest(fam + ".g_out", fake)
        rec["d_out"] = {"vals": dout.detach().double().tolist()}
        rec["g_grads"] = digest_dict(fam + ".gg.", [(k, p.grad) for k, p in g.named_parameters()])
        rec["d_grads"] = digest_dict(fam + ".dg.", [(k, p.grad) for k, p in d.named_parameters()])
        rec["d_xgrad"] = digest(fam + ".d_xgrad", x.grad)
        rec["g_post"] = digest_dict(fam + ".gpost.", g.state_dict().items())
        rec["d_post"] = digest_dict(fam + ".dpost.", d.state_dict().items())
        out[fam] = rec
    return out


# --------------------------------------------------------------------------------------------
# real trainers under a synthetic data_pre
# --------------------------------------------------------------------------------------------
class Args:
    def __init__(self, **k):
        self.__dict__.update(k)


class SynthPre:
    """duck type of preprocess.*DataPreprocessor: get_data_loader() -> (batches, metric_source)."""

    def __init__(self, batches):
        self.batches = batches
        self.idx_to_labels = {i: str(i) for i in range(100)}

    def get_data_loader(self):
        return self.batches, None


class FakeMetrics:
    def __init__(self, *_):
        pass

    def inception_score(self, *_a, **_k):
        return 1.0

    def fid(self, *_a, **_k):
        return 1.0

    def intra_fid(self, *_a, **_k):
        return 1.0


def run_trainer(fam, B, steps, lr, tmp):
    """Runs the reference's own <X>Trainer.train() and records per-step quantities through wrappers
    around objects the trainer exposes (criterion, optimizers, compute_gradient_penalty)."""
    import matplotlib.pyplot as plt
    from logger.main_logger import MainLogger
    MainLogger._instance = None
    MainLogger._initialized = False
    import logging
    logging.getLogger("main").handlers.clear()
    if fam == "dcgan":
        from model import DCGAN as M
        from train import dcgan_trainer as T
        TR = T.DCGANTrainer
    else:
        from model import CGAN as M
        from train import cgan_trainer as T
        TR = T.CGANTrainer
    T.Metrics = FakeMetrics
    imgs = synth_images(B * steps)
    if fam == "dcgan":
        batches = [(imgs[i * B:(i + 1) * B],) for i in range(steps)]
    else:
        oh, _ = synth_onehot(B * steps)
        batches = [(imgs[i * B:(i + 1) * B], oh[i * B:(i + 1) * B]) for i in range(steps)]
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        args = Args(epoch=1, max_learning_rate=lr, model_path="golden", log_file=0,
                    save_path=os.path.join(tmp, "save", fam, "golden"), batch_size=B, num_worker=0)
        torch.manual_seed(MODEL_SEED)
        g, d = M.Generator(), M.Discriminator()
        tr = TR(args, g, d, SynthPre(batches))
        rec = {"B": B, "steps": steps, "lr": lr,
               "init_g": digest_dict(f"{fam}.g.", g.state_dict().items()),
               "init_d": digest_dict(f"{fam}.d.", d.state_dict().items()), "step": []}
        cur = {"crit": [], "gp": None}

        crit = tr.criterion

        def crit_wrap(o, t):
            l = crit(o, t)
            cur["crit"].append({"out": o.detach().double().tolist(), "loss": float(l.detach())})
            return l
        tr.criterion = crit_wrap
        gp_fn = tr.compute_gradient_penalty

        def gp_wrap(*a):
            v = gp_fn(*a)
            cur["gp"] = float(v.detach())
            return v
        tr.compute_gradient_penalty = gp_wrap
        od_step, og_step = tr.optimizer_d.step, tr.optimizer_g.step

        def od_wrap(*a, **k):
            cur["d_grads"] = digest_dict(f"{fam}.dg.", [(n, p.grad) for n, p in d.named_parameters()])
            r = od_step(*a, **k)
            cur["d_post"] = digest_dict(f"{fam}.dpost.", d.state_dict().items())
            return r

        def og_wrap(*a, **k):
            cur["g_grads"] = digest_dict(f"{fam}.gg.", [(n, p.grad) for n, p in g.named_parameters()])
            r = og_step(*a, **k)
            cur["g_post"] = digest_dict(f"{fam}.gpost.", g.state_dict().items())
            # D's BN running stats move once more in the G phase (4th D pass)
            cur["d_post_bn"] = digest_dict(f"{fam}.dpostbn.", [(n, b) for n, b in d.named_buffers()])
            rec["step"].append(dict(cur))
            cur["crit"] = []
            return r
        tr.optimizer_d.step, tr.optimizer_g.step = od_wrap, og_wrap
        captured = {}
        plot = plt.plot

        def plot_wrap(x, y, *a, **k):
            captured[k.get("label", "?")] = [float(v) for v in y]
            return plot(x, y, *a, **k)
        plt.plot = plot_wrap
        try:
            tr.train()
        finally:
            plt.plot = plot
            plt.close("all")
        rec["losses_d"] = captured.get("Discriminator Loss")
        rec["losses_g"] = captured.get("Generator Loss")
        rec["final_g"] = digest_dict(f"{fam}.gfin.", g.state_dict().items())
        rec["final_d"] = digest_dict(f"{fam}.dfin.", d.state_dict().items())
        rec["saved"] = sorted(os.path.relpath(os.path.join(r, f), tmp) for r, _, fs in os.walk(tmp) for f in fs)
        pts = [p for p in rec["saved"] if p.endswith(".pt")]
        if pts:
            ck = torch.load(os.path.join(tmp, pts[0]), weights_only=False)
            rec["ckpt_keys"] = sorted(ck.keys())
            rec["ckpt_g_keys"] = list(ck["model_g"].keys())
            rec["ckpt_d_keys"] = list(ck["model_d"].keys())
        return rec
    finally:
        os.chdir(cwd)


def gen_steps(fam):
    import tempfile
    out = {}
    cfgs = [(8, 3, 2e-4), (64, 3, 2e-4)] if fam == "dcgan" else [(8, 2, 2e-4), (32, 2, 2e-4)]
    for B, steps, lr in cfgs:
        with tempfile.TemporaryDirectory() as tmp:
            out[f"B{B}"] = run_trainer(fam, B, steps, lr, tmp)
    if fam == "dcgan":
        with tempfile.TemporaryDirectory() as tmp:
            r = run_trainer(fam, 8, 4, 0.1, tmp)       # CLI default lr: pins the -100 clamp plateau
            out["B8_lr0.1"] = {k: r[k] for k in ("B", "steps", "lr", "losses_d", "losses_g")}
            out["B8_lr0.1"]["crit"] = [[c["loss"] for c in s["crit"]] for s in r["step"]]
            out["B8_lr0.1"]["gp"] = [s["gp"] for s in r["step"]]
    return out


# --------------------------------------------------------------------------------------------
# metrics arithmetic (reference's Metrics methods, unmodified, on supplied features)
# --------------------------------------------------------------------------------------------
def gen_metrics():
    import metrics as RM
    rng = np.random.default_rng(7)
    real = (1.5 * rng.standard_normal((5000, 100)) + 0.2).astype(np.float32)
    fake = rng.standard_normal((1000, 100)).astype(np.float32)
    real_targets = rng.integers(0, 100, size=5000).tolist()
    m = RM.Metrics.__new__(RM.Metrics)
    # the superclass table is data inside Metrics.__init__; rebuild the two index maps the same way
    src = {}
    tbl = [[4, 30, 55, 72, 95], [1, 32, 67, 73, 91], [54, 62, 70, 82, 92], [9, 10, 16, 28, 61], [0, 51, 53, 57, 83],
           [22, 39, 40, 86, 87], [5, 20, 25, 84, 94], [6, 7, 14, 18, 24], [3, 42, 43, 88, 97], [12, 17, 37, 68, 76],
           [23, 33, 49, 60, 71], [15, 19, 21, 31, 38], [34, 63, 64, 66, 75], [26, 45, 77, 79, 99], [2, 11, 35, 46, 98],
           [27, 29, 44, 78, 93], [36, 50, 65, 74, 80], [47, 52, 56, 59, 96], [8, 13, 48, 58, 90], [41, 69, 81, 85, 89]]
    for s, cl in enumerate(tbl):
        for c in cl:
            src[c] = s
    fake_targets = [i for i in range(100) for _ in range(10)]
    m.real_superclass_idx = {s: [i for i, t in enumerate(real_targets) if src[t] == s] for s in range(20)}
    m.fake_superclass_idx = {s: [i for i, t in enumerate(fake_targets) if src[t] == s] for s in range(20)}
    m.real_features = real
    m.device = torch.device("cpu")

    def extract(images, real=False, softmax=False):
        feats = np.vstack([b.numpy() for b in images])
        if softmax:
            feats = torch.softmax(torch.from_numpy(feats), dim=1).numpy()
        return feats
    m._Metrics__extract_features = extract
    ft = torch.from_numpy(fake)
    dl = torch.utils.data.DataLoader(ft, batch_size=128, shuffle=False)
    rec = {"recipe": {"rng": 7, "real": "1.5*N(0,1)+0.2 [5000,100] f32", "fake": "N(0,1) [1000,100] f32",
                      "real_targets": "integers(0,100,5000)"},
           "is": float(m.inception_score(dl)), "fid": float(m.fid(dl)), "intra_fid": float(m.intra_fid(ft))}
    dl64 = torch.utils.data.DataLoader(ft[:64], batch_size=64)
    rec["is64"] = float(m.inception_score(dl64))
    rec["fid64"] = float(m.fid(dl64))
    return rec


# --------------------------------------------------------------------------------------------
# reference vs itself: chaotic-trajectory noise floor
# --------------------------------------------------------------------------------------------
def gen_selfdiv(steps=30, B=64):
    from model import DCGAN as M
    import copy
    torch.manual_seed(MODEL_SEED)
    g0, d0 = M.Generator(), M.Discriminator()
    g0.apply(M.weights_init)
    d0.apply(M.weights_init)
    imgs = synth_images(B * 4)
    gen = torch.Generator().manual_seed(31)
    noise = [(torch.randn(B, 3, 64, 64, generator=gen), torch.randn(B, 100, 1, 1, generator=gen),
              torch.randn(B, 3, 64, 64, generator=gen), torch.rand(B, 1, 1, 1, generator=gen)) for _ in range(steps)]
    crit = torch.nn.BCELoss()

    def run(nthreads):
        torch.set_num_threads(nthreads)
        g, d = copy.deepcopy(g0), copy.deepcopy(d0)
        og = torch.optim.Adam(g.parameters(), lr=2e-4, betas=[0.5, 0.999])
        od = torch.optim.Adam(d.parameters(), lr=2e-4, betas=[0.5, 0.999])
        ld, lg = [], []
        for s in range(steps):
            n1, z, n2, al = noise[s]
            real = imgs[(s % 4) * B:(s % 4 + 1) * B]
            # statements of train/dcgan_trainer.py:155-189 with the RNG draws replaced by the shared tensors
            d.zero_grad()
            label = torch.full((B,), 0.9)
            real = 0.9 * real + 0.1 * n1
            out = d(real).view(-1)
            e_real = crit(out, label)
            e_real.backward()
            fake = g(z)
            label.fill_(0.1)
            fake = 0.9 * fake + 0.1 * n2
            out = d(fake.detach()).view(-1)
            e_fake = crit(out, label)
            e_fake.backward()
            inter = (al * real + (1 - al) * fake).requires_grad_(True)
            di = d(inter)
            gr = torch.autograd.grad(di, inter, torch.ones_like(di), create_graph=True, retain_graph=True)[0]
            gp = ((gr.view(B, -1).norm(2, dim=1) - 1) ** 2).mean()
            e_d = e_real + e_fake + 10.0 * gp
            od.step()
            g.zero_grad()
            label.fill_(0.9)
            out = d(fake).view(-1)
            e_g = crit(out, label)
            e_g.backward()
            og.step()
            ld.append(float(e_d))
            lg.append(float(e_g))
        return ld, lg
    d8, g8 = run(8)
    d1, g1 = run(1)
    torch.set_num_threads(8)
    return {"B": B, "steps": steps, "loss_d_8t": d8, "loss_g_8t": g8, "loss_d_1t": d1, "loss_g_1t": g1,
            "rel_d": [abs(a - b) / max(abs(a), 1e-12) for a, b in zip(d8, d1)],
            "rel_g": [abs(a - b) / max(abs(a), 1e-12) for a, b in zip(g8, g1)]}


# --------------------------------------------------------------------------------------------
# the plain latent entry points on the GPU, bit for bit (the project's own results at a recorded commit; no reference involved)
# --------------------------------------------------------------------------------------------
LATENT_LOSS_CASES = [(n, hw, p) for n, hw in ((1, 64), (5, 4096)) for p in ("f32", "bf16")]
LATENT_ENGINES = [(f, p) for f in ("dcgan", "cgan") for p in ("bf16", "f32")]          # tests/test_critic_grad_gpu.py ENGINES
_latent_engines = {}


def sha256_bytes(t):
    """SHA-256 of a tensor's raw bytes (.cpu() waits for the stream that wrote it)"""
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def latent_loss_bits(n, hw, prec, ex):
    """{g_raw, loss: digest} of jck_latent_loss (ex: jck_latent_loss_ex without weight and image gradient) on seeded inputs:
    hw = 64 is less than one pass of the kernel's 256-thread loop, hw = 4096 is 16 passes"""
    from hipgan import PREC_BF16, PREC_F32, lib
    from hipgan._lib import cur_stream
    pc, dt = (PREC_BF16, torch.bfloat16) if prec == "bf16" else (PREC_F32, torch.float32)
    g = torch.Generator().manual_seed(51)
    x = torch.tanh(torch.randn(n, hw, 4, generator=g)).to(dt).cuda()
    t = (torch.rand(n, 3, hw, generator=g) * 2 - 1).cuda()
    graw, loss = torch.zeros(n, hw, 4, dtype=dt, device="cuda"), torch.zeros(n, device="cuda")
    if ex:
        lib.jck_latent_loss_ex(pc, x, t, None, None, graw, loss, n, hw, cur_stream())
    else:
        lib.jck_latent_loss(pc, x, t, graw, loss, n, hw, cur_stream())
    return {"g_raw": sha256_bytes(graw), "loss": sha256_bytes(loss)}


def latent_engine(family, prec):
    """a batch-8 64x64 engine as tools/project_rate.py makes it: the oracle's weights, running statistics after 30 train-mode batches"""
    if (family, prec) not in _latent_engines:
        from hipgan.engine import CganEngine, DcganEngine
        from oracle.gan_oracle import GanOracle
        orc = GanOracle(family, lr=2e-4, seed=12345)
        eng = (CganEngine if family == "cgan" else DcganEngine)(batch=8, prec=prec)
        eng.load_state(orc.g, orc.d)
        zz = torch.randn(8, 100, generator=torch.Generator().manual_seed(1))
        lab = synth_onehot(8)[0] if family == "cgan" else None
        for _ in range(30):
            eng.sample(zz, lab)
        _latent_engines[family, prec] = eng
    return _latent_engines[family, prec]


def latent_engine_bits(family, prec, ex):
    """digests of jck_engine_latent_grad's (loss, dz) and of (z, m, v, loss_hist) after a 3-step jck_engine_project (lr 0.05, prior
    0.01), n = 5 of 8 (a ragged batch); ex: the same through the _ex entry points with no weight and no critic"""
    from hipgan import lib
    from hipgan._lib import cur_stream
    eng = latent_engine(family, prec)
    n, steps = 5, 3
    g = torch.Generator().manual_seed(DATA_SEED + 2)
    z0 = torch.randn(n, 100, generator=g).cuda()
    t = (torch.rand(n, 3, 64, 64, generator=g) * 2 - 1).cuda()
    lab = synth_onehot(n, DATA_SEED + 3)[0].cuda() if family == "cgan" else None
    f = lambda *sh: torch.zeros(*sh, device="cuda")
    loss, dz, z, m, v, hist = f(n), f(n, 100), z0.clone(), f(n, 100), f(n, 100), f(steps, n)
    if ex:
        lib.jck_engine_latent_grad_ex(eng._h, z0, lab, t, None, 0, 0.0, n, loss, None, None, dz, cur_stream())
        lib.jck_engine_project_ex(eng._h, z, lab, t, n, steps, 0.05, 0.01, None, 0, 0.0, m, v, 0, hist, None, cur_stream())
    else:
        lib.jck_engine_latent_grad(eng._h, z0, lab, t, n, loss, dz, cur_stream())
        lib.jck_engine_project(eng._h, z, lab, t, n, steps, 0.05, 0.01, m, v, 0, hist, cur_stream())
    named = {"latent_grad.loss": loss, "latent_grad.dz": dz, "project.z": z, "project.m": m, "project.v": v, "project.loss_hist": hist}
    return {k: sha256_bytes(x) for k, x in named.items()}


def gen_latent_plain_bits(commit):
    assert torch.cuda.is_available(), "latent_plain_bits records what the GPU computes"
    assert commit, "--commit: name the commit the library under test was built from"
    for p in (os.path.dirname(os.path.dirname(HERE)), os.path.join(os.path.dirname(os.path.dirname(HERE)), "jck-generation_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    rec = {"commit": commit, "device": torch.cuda.get_device_name(0), "entry_points": "plain (jck_latent_loss, jck_engine_latent_grad, jck_engine_project)"}
    rec["latent_loss"] = {f"{n}x{hw}-{p}": latent_loss_bits(n, hw, p, False) for n, hw, p in LATENT_LOSS_CASES}
    rec["engine"] = {f"{f}-{p}": latent_engine_bits(f, p, False) for f, p in LATENT_ENGINES}
    return rec


# --------------------------------------------------------------------------------------------
# the inference paths beside the plain ones, bit for bit: the _ex / _fm latent entry points with their objective terms on,
# jck_engine_score, jck_engine_features and the Python layer over them (again the project's own results at a recorded commit)
# --------------------------------------------------------------------------------------------
INFER_ENGINES = LATENT_ENGINES + [(f, "bf16x3") for f in ("dcgan", "cgan") if (f, "bf16x3") not in LATENT_ENGINES]
INFER_GROUPS = ("latent_ex", "latent_fm", "score", "features", "python")
# name: (target, per-pixel weight, critic mode, critic weight)
INFER_EX_CASES = {"weight": (True, True, 0, 0.0), "nsgan": (True, False, 1, 0.003), "logit_no_target": (False, False, 2, 1.0),
                  "weight_nsgan": (True, True, 1, 0.003)}
# name: (target, feature stage, critic mode, critic weight); the feature weight is 0.5
INFER_FM_CASES = {"stage0": (True, 0, 0, 0.0), "deepest_no_target": (False, -1, 0, 0.0), "stage1_nsgan": (True, 1, 1, 0.003)}


def infer_inputs(family, n=5):
    """seeded rows of an inference call: z, target, per-pixel weight (a block of unknown pixels), feature target, instance noise, labels"""
    g = torch.Generator().manual_seed(DATA_SEED + 4)
    z = torch.randn(n, 100, generator=g)
    t, ft = torch.rand(n, 3, 64, 64, generator=g) * 2 - 1, torch.rand(n, 3, 64, 64, generator=g) * 2 - 1
    w = torch.rand(n, 64, 64, generator=g)
    w[:, 16:40, 20:48] = 0.0
    nz = torch.randn(n, 3, 64, 64, generator=g)
    lab = synth_onehot(n, DATA_SEED + 5)[0].cuda() if family == "cgan" else None
    return z.cuda(), t.cuda(), w.cuda(), ft.cuda(), nz.cuda(), lab


def infer_bits(family, prec, group):
    """{"case.output": digest} of one group of calls on latent_engine(family, prec), n = 5 of 8; a 3-step projection at lr 0.05, prior 0.01"""
    from hipgan import lib
    from hipgan._lib import cur_stream
    eng = latent_engine(family, prec)
    n, steps, out = 5, 3, {}
    z0, t, w, ft, nz, lab = infer_inputs(family, n)
    f = lambda *sh: torch.zeros(*sh, device="cuda")
    put = lambda case, named: out.update({f"{case}.{k}": sha256_bytes(x) for k, x in named.items()})

    def latent(case, tt, ww, mode, cw, fm=None):
        loss, term, logit, fterm, dz = f(n), f(n), f(n), f(n), f(n, 100)
        z, m, v, hist, thist, fhist = z0.clone(), f(n, 100), f(n, 100), f(steps, n), f(steps, n), f(steps, n)
        if fm is None:
            lib.jck_engine_latent_grad_ex(eng._h, z0, lab, tt, ww, mode, cw, n, loss, term, logit, dz, cur_stream())
            lib.jck_engine_project_ex(eng._h, z, lab, tt, n, steps, 0.05, 0.01, ww, mode, cw, m, v, 0, hist, thist, cur_stream())
        else:
            lib.jck_engine_latent_grad_fm(eng._h, z0, lab, tt, ww, mode, cw, n, loss, term, logit, dz, cur_stream(), ft, fm, 0.5, fterm)
            lib.jck_engine_project_fm(eng._h, z, lab, tt, n, steps, 0.05, 0.01, ww, mode, cw, m, v, 0, hist, thist, cur_stream(), ft, fm, 0.5,
                                      fhist)
        named = {"loss": loss, "term": term, "logit": logit, "dz": dz, "z": z, "m": m, "v": v, "loss_hist": hist, "term_hist": thist}
        if fm is not None:
            named.update({"fterm": fterm, "fterm_hist": fhist})
        put(case, named)

    if group == "latent_ex":
        for case, (has_t, has_w, mode, cw) in INFER_EX_CASES.items():
            latent(case, t if has_t else None, w if has_w else None, mode, cw)
    elif group == "latent_fm":
        for case, (has_t, stage, mode, cw) in INFER_FM_CASES.items():
            latent(case, t if has_t else None, None, mode, cw, fm=stage)
    elif group == "score":
        for case, (x, noise) in {"images": (t, None), "images_noise": (t, nz), "current": (None, None)}.items():
            if x is None:
                lib.jck_engine_sample_ex(eng._h, z0, lab, n, 1, None, None, cur_stream())          # JCK_SAMPLE_EVAL
            logit, prob = f(n), f(n)
            lib.jck_engine_score(eng._h, x, noise, lab, n, logit, prob, cur_stream())
            put(case, {"logit": logit, "prob": prob})
    elif group == "features":
        for case, (grid, mode) in {"grid1_max": (1, 0), "grid4_mean": (4, 1)}.items():
            F = lib.jck_engine_feature_dim(eng._h, grid)
            rows = f(n, F)
            lib.jck_engine_features(eng._h, t, n, grid, mode, rows, F, cur_stream())
            put(case, {"rows": rows})
    elif group == "python":
        put("latent_grad", dict(zip(("loss", "dz"), eng.latent_grad(z0, t, lab))))
        put("latent_grad_critic", dict(zip(("loss", "term", "logit", "dz"),
                                           eng.latent_grad(z0, t, lab, weight=w, critic="nsgan", critic_weight=0.003))))
        put("latent_grad_feature", eng.latent_grad(z0, t, lab, feature_target=ft, feature_weight=0.5, feature_stage=1))
        put("critic_grad", dict(zip(("logit", "term", "dz"), eng.critic_grad(z0, lab))))
        z, hist = eng.project(t, lab, steps=steps, lr=0.05, prior=0.01, z0=z0, critic="nsgan", critic_weight=0.003, feature_target=ft,
                              feature_weight=0.5, feature_stage=1)
        put("project", {"z": z, "loss_hist": hist, "state.m": eng.project_state["m"], "state.v": eng.project_state["v"],
                        "term": eng.project_term, "fterm": eng.project_fterm})
        put("refine", dict(zip(("z", "before", "after"), eng.refine(z0, lab, steps=2))))
    else:
        raise KeyError(group)
    return out


def gen_infer_bits(commit):
    assert torch.cuda.is_available(), "infer_bits records what the GPU computes"
    assert commit, "--commit: name the commit the library under test was built from"
    for p in (os.path.dirname(os.path.dirname(HERE)), os.path.join(os.path.dirname(os.path.dirname(HERE)), "jck-generation_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    rec = {"commit": commit, "device": torch.cuda.get_device_name(0), "engine": {}, "not_reproducible": []}
    for fam, prec in INFER_ENGINES:
        for group in INFER_GROUPS:
            a, b = infer_bits(fam, prec, group), infer_bits(fam, prec, group)      # a key whose two digests differ is not written
            rec["not_reproducible"] += [f"{fam}-{prec}.{group}.{k}" for k in a if a[k] != b[k]]
            rec["engine"].setdefault(f"{fam}-{prec}", {})[group] = {k: d for k, d in a.items() if d == b[k]}
    for k in rec["not_reproducible"]:
        print("NOT REPRODUCIBLE, left out:", k)
    return rec


# --------------------------------------------------------------------------------------------
# generate.py's parser as a table: which command lines it accepts, and the namespace of each (the project's own, on the CPU)
# --------------------------------------------------------------------------------------------
CLI_MODELS = ("DCGAN", "CGAN")
CLI_UNITS_A = [
    "--num 5", "--num 0", "-b 8", "-b 0", "--seed 3", "--truncation 0.7", "--truncation 0", "--bn batch", "--which ema", "--calibrate 2",
    "--calibrate -1", "--classes 3,17", "--classes 3", "--interpolate 2:4", "--project f.npz", "--project_steps 7", "--project_steps 0",
    "--project_lr 0.1", "--project_lr 0", "--project_prior 0.5", "--project_prior -1", "--score", "--select top", "--select top --oversample 4",
    "--select drs --oversample 4", "--oversample 4", "--select top --oversample 0", "--score_images f.npz", "--neighbours r.npz", "--k 3", "--k 9",
    "--space d", "--space pixel", "--features f.npz", "--feature_grid 2", "--feature_pool mean", "--probe tr.npz", "--probe_test te.npz",
    "--probe tr.npz --probe_test te.npz", "--inpaint f.npz", "--mask center:32", "--inpaint f.npz --mask center:32", "--critic_weight 0",
    "--critic_weight 0.5", "--critic_weight -1", "--refine 5", "--refine 0", "--refine_lr 0.1", "--refine_lr 0", "--project_feature_weight 10",
    "--project_feature_weight -1", "--project_feature_weight inf", "--anomaly f.npz", "--anomaly_lam 0.3", "--anomaly_lam 1", "--anomaly_stage 2",
    "--anomaly_stage 5", "--prec f32"]
CLI_SELECTORS_B = [
    "--project f.npz", "--score_images f.npz", "--features f.npz", "--probe tr.npz --probe_test te.npz", "--inpaint f.npz --mask center:32",
    "--anomaly f.npz", "--interpolate 2:4", "--select top --oversample 4", "--select drs --oversample 4", "--refine 5", "--score",
    "--neighbours r.npz"]
CLI_UNITS_B = [
    "--num 5", "--truncation 0.7", "--bn batch", "--calibrate 2", "--classes 3", "--project_steps 7", "--project_prior 0.5", "--score",
    "--neighbours r.npz", "--k 3", "--space d", "--feature_grid 2", "--feature_pool mean", "--critic_weight 0.5", "--refine 5", "--refine_lr 0.1",
    "--project_feature_weight 10", "--anomaly_lam 0.3", "--anomaly_stage 2", "--interpolate 2:4", "--select top --oversample 4", "--prec f32"]


def cli_lines(which):
    """the command lines of set "A" (every 0, 1 or 2 of CLI_UNITS_A) or "B" (a complete selector and every pair of CLI_UNITS_B but
    itself) as strings of units, in the fixture's order; each is tried under -m DCGAN and -m CGAN"""
    from itertools import combinations
    if which == "A":
        return [" ".join(c) for r in (0, 1, 2) for c in combinations(CLI_UNITS_A, r)]
    return [" ".join((s,) + c) for s in CLI_SELECTORS_B for c in combinations([u for u in CLI_UNITS_B if u != s], 2)]


def cli_namespace(model, line):
    """{attribute: repr(value)} of generate.get_arg_parse on one command line, or None where the parser refuses it"""
    import contextlib
    import io
    import generate
    argv = ["-m", model, "--checkpoint", "c.pt", "--out", "o"] + line.split()
    try:
        with contextlib.redirect_stderr(io.StringIO()):
            a = generate.get_arg_parse(argv)
    except SystemExit:
        return None
    return {k: repr(v) for k, v in vars(a).items()}


def cli_digest(ns, attrs):
    """"x" for a refused line, else 12 hex digits of the SHA-256 of the namespace's `attrs` as sorted JSON of repr values"""
    if ns is None:
        return "x"
    return hashlib.sha256(json.dumps({k: ns[k] for k in attrs}, sort_keys=True).encode()).hexdigest()[:12]


def cli_table(attrs=None):
    """{"attrs", "A": {model: [digest per line of cli_lines("A")]}, "B": ..., "full": {"model: line": namespace or "x"}} - the full
    namespace only of the empty and the one-unit lines, so that a difference can be read.  attrs None: every attribute the namespace has."""
    if attrs is None:
        attrs = sorted(cli_namespace("DCGAN", ""))
    rec = {"attrs": list(attrs), "A": {}, "B": {}, "full": {}}
    for which in ("A", "B"):
        for model in CLI_MODELS:
            nss = [cli_namespace(model, line) for line in cli_lines(which)]
            rec[which][model] = [cli_digest(ns, attrs) for ns in nss]
            if which == "A":
                for line, ns in zip(cli_lines("A"), nss):
                    if line in [""] + CLI_UNITS_A:
                        rec["full"][f"{model}: {line}"] = "x" if ns is None else {k: ns[k] for k in attrs}
    return rec


def _project_paths():
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "jck-generation_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def gen_generate_cli(commit):
    assert commit, "--commit: name the commit whose parser is recorded"
    _project_paths()
    rec = {"commit": commit, **cli_table()}
    for which in ("A", "B"):
        n = sum(len(v) for v in rec[which].values())
        print(f"set {which}: {n} lines, {sum(d != 'x' for v in rec[which].values() for d in v)} accepted")
    return rec


# --------------------------------------------------------------------------------------------
# generate.py end to end on the GPU, bit for bit: every file and the stdout line of one run per mode and sampling strategy
# (the project's own results at a recorded commit).  Shapes: -b 8, 64x64, 5 or 20 images cross a chunk edge; 3 projection steps.
# --------------------------------------------------------------------------------------------
# name: (checkpoint, arguments; "@a" / "@c" / "@q": the images.npz of run a / c, and a's pictures with an `anomalous` array)
GENERATE_RUNS = {
    "a": ("plain", "--num 20 --seed 3 --truncation 0.7"),
    "b": ("plain", "--num 20 --seed 3 --truncation 0.7 --bn batch"),
    "c": ("cgan", "-m CGAN --num 3 --classes 3,17"),
    "d": ("cgan", "-m CGAN --interpolate 3:4 --classes 3,17"),
    "e": ("ema", "--which ema --calibrate 2 --num 5"),
    "f": ("plain", "--num 5 --score"),
    "g": ("plain", "--num 5 --select top --oversample 3 --score"),
    "h": ("plain", "--num 5 --select drs --oversample 4"),
    "i": ("plain", "--num 5 --refine 2"),
    "j": ("plain", "--project @a --project_steps 3"),
    "k": ("plain", "--project @a --project_steps 3 --project_feature_weight 10"),
    "l": ("cgan", "-m CGAN --project @c"),
    "m": ("plain", "--inpaint @a --mask center:32 --project_steps 3"),
    "n": ("plain", "--inpaint @a --mask center:32 --project_steps 3 --critic_weight 0"),
    "o": ("plain", "--anomaly @q --project_steps 3 --anomaly_lam 0.3 --anomaly_stage 1"),
    "p": ("plain", "--score_images @a --neighbours @a --k 2"),
    "q": ("plain", "--num 5 --neighbours @a --space d --feature_grid 2 --k 2"),
    "r": ("plain", "--features @a --feature_grid 2 --feature_pool mean"),
    "s": ("plain", "--probe @c --probe_test @c --k 3"),
}
GENERATE_HOST_ARRAYS = ("z", "labels", "known", "order", "layout")      # (of these only a sampling run's z is never touched by the device)
DRAW_CAP = "(cap 50 * n)"


def generate_workdir(d):
    """Makes directory d the place the runs of GENERATE_RUNS are started from: the three checkpoints of gpu_util.make_checkpoints, the
    outputs of runs a and c (which the other runs read) and q.npz -> {"a": digests of run a, "c": of run c}"""
    from gpu_util import make_checkpoints
    make_checkpoints(d)
    done = {k: generate_run(d, k) for k in ("a", "c")}
    with np.load(os.path.join(str(d), "a", "images.npz")) as f:
        np.savez(os.path.join(str(d), "q.npz"), images=f["images"], anomalous=np.arange(f["images"].shape[0]) % 3 == 0)
    return done


def generate_run(d, name):
    """{"file.npz:array" | "file.png" | "file.json" | "stdout": SHA-256} of run `name`, started in directory d (generate_workdir) with
    relative paths, so that the printed line names no temporary directory.  An array's digest covers dtype, shape and raw bytes."""
    import contextlib
    import io
    import generate
    ck, line = GENERATE_RUNS[name]
    argv = ["--checkpoint", ck + ".pt", "-b", "8", "--out", name] + [{"@a": "a/images.npz", "@c": "c/images.npz", "@q": "q.npz"}.get(t, t)
                                                                    for t in line.split()]
    cwd, buf = os.getcwd(), io.StringIO()
    os.chdir(str(d))
    try:
        with contextlib.redirect_stdout(buf):
            assert generate.main(argv) == 0
        out = {"stdout": hashlib.sha256(buf.getvalue().encode()).hexdigest()}
        for fn in sorted(os.listdir(name)):
            path = os.path.join(name, fn)
            if fn.endswith(".npz"):
                with np.load(path) as f:
                    for k in f.files:
                        a = np.ascontiguousarray(f[k])
                        out[f"{fn}:{k}"] = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()
            else:
                out[fn] = hashlib.sha256(open(path, "rb").read()).hexdigest()
    finally:
        os.chdir(cwd)
    return out


def gen_generate_bits(commit):
    import tempfile
    assert torch.cuda.is_available(), "generate_bits records what the GPU computes"
    assert commit, "--commit: name the commit the library and generate.py are those of"
    _project_paths()
    from hipgan._lib import JckError
    rec = {"commit": commit, "device": torch.cuda.get_device_name(0), "runs": {}, "not_reproducible": [], "left_out": {}}
    with tempfile.TemporaryDirectory() as d:
        first = generate_workdir(d)
        for name in GENERATE_RUNS:
            try:
                a, b = first.get(name) or generate_run(d, name), generate_run(d, name)      # a key whose two digests differ is not written
            except JckError as e:
                assert name == "h" and DRAW_CAP in str(e), (name, e)                       # only rejection sampling's draw cap excuses a run
                rec["left_out"][name] = str(e)
                continue
            assert set(a) == set(b), (name, sorted(set(a) ^ set(b)))
            rec["not_reproducible"] += [f"{name}.{k}" for k in a if a[k] != b[k]]
            rec["runs"][name] = {k: v for k, v in a.items() if v == b[k]}
    bad, total = rec["not_reproducible"], sum(len(r) for r in rec["runs"].values()) + len(rec["not_reproducible"])
    for k in bad:
        print("NOT REPRODUCIBLE, left out:", k)
    assert not [k for k in bad if k.split(":")[-1] in GENERATE_HOST_ARRAYS], "a host-made array did not repeat"
    assert len(bad) <= 0.05 * total, f"{len(bad)} of {total} digests did not repeat"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--commit", default="", help="the project's own fixtures: the commit the code recorded is that of")
    a = ap.parse_args()
    own = {"latent_plain_bits": gen_latent_plain_bits, "infer_bits": gen_infer_bits, "generate_cli": gen_generate_cli,
           "generate_bits": gen_generate_bits}
    if a.only in own:                                  # the project's own results, not the reference's
        rec = own[a.only](a.commit)
        rec["_meta"] = {"torch": torch.__version__, "generator": "tests/golden/make_golden.py", "model_seed": MODEL_SEED, "data_seed": DATA_SEED}
        with open(os.path.join(HERE, a.only + ".json"), "w") as f:
            json.dump(rec, f, indent=1)
        print(a.only, "->", os.path.getsize(os.path.join(HERE, a.only + ".json")), "bytes")
        return
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    install_stubs()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    jobs = {"modules": gen_modules, "dcgan_steps": lambda: gen_steps("dcgan"),
            "cgan_steps": lambda: gen_steps("cgan"), "metrics": gen_metrics, "selfdiv": gen_selfdiv}
    for name, fn in jobs.items():
        if a.only and name not in a.only.split(","):
            continue
        rec = fn()
        rec["_meta"] = {"torch": torch.__version__, "threads": torch.get_num_threads(),
                        "generator": "tests/golden/make_golden.py", "model_seed": MODEL_SEED, "data_seed": DATA_SEED}
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump(rec, f)
        print(name, "->", os.path.getsize(os.path.join(HERE, name + ".json")), "bytes")


if __name__ == "__main__":
    main()
