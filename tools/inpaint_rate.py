"""Iterations per second of a masked projection with and without the critic (DcganEngine.project(weight=..., critic=...): bf16, 64x64,
batch 64 and 256 by default) next to the plain projection of tools/project_rate.py measured in the same run.  One iteration is one
Adam update of every latent of the batch; with the critic it adds the eval-mode discriminator's forward on G(z), the head's input
gradient, the leaky masked dgrads down to an image gradient.

Protocol as tools/project_rate.py: `--warmup` calls, then `--repeats` groups, each ONE jck_engine_project_ex call of `--steps`
iterations timed with device events around it; the median group's rate and the spread (min, max), and per iteration the device time
next to the host's enqueue time: where the two meet the rate is the host's, not the kernels'.  One JSON line per batch and form.

    timeout -k 10 300 python tools/inpaint_rate.py
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jck-generation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMS = ("plain", "masked", "masked+critic")
# launches per iteration of a bf16 64x64 DCGAN: 5 generator products, the loss, 4 masked dgrads, the dz product, Adam;
# the critic adds 4 x 2 stage launches, the head, jck_critic_ds, the head's input gradient, jck_leaky_affine_bwd, 3 jck_conv_up_mask, jck_conv_up
LAUNCHES = {"plain": 12, "masked": 12, "masked+critic": 28}


def measure(eng, batch, steps, warmup, repeats, form):
    from hipgan._lib import cur_stream, lib
    from hipgan.inpaint import importance_weights, parse_mask
    g = torch.Generator().manual_seed(0)
    z = torch.randn(batch, 100, generator=g).cuda()
    with torch.no_grad():
        target = eng.sample(torch.randn(batch, 100, generator=g).cuda(), bn="running").clone()      # pictures the generator can make
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    hist = torch.empty(steps, batch, device="cuda")
    w = None
    if form != "plain":
        w = importance_weights(parse_mask("center:32", 64), 7).unsqueeze(0).expand(batch, -1, -1).contiguous().cuda()
    mode, cw = (1, 0.003) if form == "masked+critic" else (0, 0.0)

    def call(t0):
        if form == "plain":
            lib.jck_engine_project(eng._h, z, None, target, batch, steps, 0.05, 0.0, m, v, t0, hist, cur_stream())
        else:
            lib.jck_engine_project_ex(eng._h, z, None, target, batch, steps, 0.05, 0.0, w, mode, cw, m, v, t0, hist, None, cur_stream())
    first = None
    for k in range(warmup):
        call(k * steps)
        if first is None:
            first = float(hist[0].mean())              # the loss at the random start
    torch.cuda.synchronize()
    rates, host, dev = [], [], []
    for k in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call((warmup + k) * steps)
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        rates.append(steps / (ms * 1e-3))
        host.append((t1 - t0) * 1e3 / steps)
        dev.append(ms / steps)
    rates.sort(), host.sort(), dev.sort()
    k = len(rates) // 2
    return {"iterations_per_s": round(rates[k], 1), "min": round(rates[0], 1), "max": round(rates[-1], 1),
            "device_ms_per_iteration": round(dev[k], 4), "host_enqueue_ms_per_iteration": round(host[k], 4),
            "host_bound": bool(host[k] >= dev[k]), "launches_per_iteration": LAUNCHES[form],
            "loss_mean_first_call": float(f"{first:.4e}"), "loss_mean_last": float(f"{float(hist[-1].mean()):.4e}")}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=100, help="iterations per timed call")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls (>= 1)")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    if args.warmup < 1 or args.steps < 1 or args.repeats < 1:
        ap.error("--warmup, --steps and --repeats must be >= 1")
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import GanOracle
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    for batch in args.batch:
        eng = DcganEngine(batch=batch, prec="bf16")
        eng.load_state(orc.g, orc.d)
        zz = torch.randn(batch, 100, generator=torch.Generator().manual_seed(1)).cuda()
        for _ in range(30):                      # running statistics fitted to the weights (with the initial (0, 1) the eval output is a flat grey)
            eng.sample(zz)
        for form in FORMS:
            r = measure(eng, batch, args.steps, args.warmup, args.repeats, form)
            print(json.dumps({"batch": batch, "prec": "bf16", "form": form, "steps_per_call": args.steps, "repeats": args.repeats, **r}), flush=True)
        del eng
    return 0


if __name__ == "__main__":
    sys.exit(main())
