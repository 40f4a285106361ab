"""Time of one projection iteration with and without the feature-matching term (DcganEngine.project(feature_target=...): bf16, 64x64,
batch 64 by default), at the deepest stage and at stage 0, next to the plain projection measured in the same run, and of
jck_feat_match alone at (batch, M_0).  One iteration is one Adam update of every latent of the batch; the feature term adds the
eval-mode discriminator's stages 0..k on G(z), jck_feat_match, the leaky masked dgrads from stage k down and jck_conv_up into an image
gradient.

Protocol as tools/inpaint_rate.py: `--warmup` calls, then `--repeats` groups, each ONE jck_engine_project_fm call of `--steps`
iterations timed with device events around it; the median group's time per iteration and the spread (min, max), next to the host's
enqueue time: where the two meet the rate is the host's, not the kernels'.  The kernel alone: `--steps` launches between two events.
One JSON line per form.

    timeout -k 10 300 python tools/feat_match_rate.py
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

# (pixel target, critic, feature stage or None): launches per iteration of a bf16 64x64 DCGAN
FORMS = {"target": (True, False, None, 12), "target + feature top": (True, False, 3, 25), "target + feature 0": (True, False, 0, 16),
         "feature top": (False, False, 3, 25), "feature 0": (False, False, 0, 16),
         "target + critic": (True, True, None, 28), "target + critic + feature top": (True, True, 3, 29)}


def timed(call, steps, warmup, repeats):
    for k in range(warmup):
        call(k)
    torch.cuda.synchronize()
    host, dev = [], []
    for k in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call(warmup + k)
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        host.append((t1 - t0) * 1e3 / steps)
        dev.append(e0.elapsed_time(e1) / steps)
    host.sort(), dev.sort()
    k = len(dev) // 2
    return {"device_ms_per_iteration": round(dev[k], 5), "min": round(dev[0], 5), "max": round(dev[-1], 5),
            "host_enqueue_ms_per_iteration": round(host[k], 5), "host_bound": bool(host[k] >= dev[k])}


def measure(eng, batch, steps, warmup, repeats, form):
    from hipgan._lib import cur_stream, lib
    pixel, critic, stage, launches = FORMS[form]
    g = torch.Generator().manual_seed(0)
    z = torch.randn(batch, 100, generator=g).cuda()
    with torch.no_grad():
        target = eng.sample(torch.randn(batch, 100, generator=g).cuda(), bn="running").clone()      # pictures the generator can make
    ft = (torch.rand(batch, 3, 64, 64, generator=g) * 2 - 1).cuda()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    hist, fh = torch.empty(steps, batch, device="cuda"), torch.zeros(steps, batch, device="cuda")
    mode, cw = (1, 0.003) if critic else (0, 0.0)

    def call(k):
        lib.jck_engine_project_fm(eng._h, z, None, target if pixel else None, batch, steps, 0.05, 0.0, None, mode, cw, m, v, k * steps, hist, None,
                                  cur_stream(), ft if stage is not None else None, -1 if stage is None else stage, 0.0 if stage is None else 1.0, fh)
    r = timed(call, steps, warmup, repeats)
    return {**r, "launches_per_iteration": launches, "loss_mean_last": float(f"{float(hist[-1].mean()):.4e}"),
            "fterm_mean_last": float(f"{float(fh[-1].mean()):.4e}")}


def measure_kernel(batch, steps, warmup, repeats):
    """jck_feat_match alone on stage 0's tensor of a 64x64 discriminator: M_0 = 32 * 32 * 64 elements per image, bf16"""
    from hipgan._lib import cur_stream, lib
    m0, c = 32 * 32 * 64, 64
    g = torch.Generator().manual_seed(0)
    a, f = (torch.randn(batch, m0, generator=g).bfloat16().cuda() for _ in range(2))
    gy, ft, scale = torch.empty_like(a), torch.empty(batch, device="cuda"), torch.rand(c, generator=g).cuda() + 0.5
    out = {}
    for acc in (0, 1):
        def call(k):
            for _ in range(steps):
                lib.jck_feat_match(0, a, f, scale, 0.2, 1.0, gy, acc, ft, batch, m0, c, cur_stream())
        r = timed(call, steps, warmup, repeats)
        byts = batch * m0 * 2 * (4 if acc else 3)
        out[acc] = {**r, "bytes": byts, "gbytes_per_s": round(byts / (r["device_ms_per_iteration"] * 1e-3) / 1e9, 1)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64])
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
        eng.score_latents(zz)                    # D's operands packed
        for form in FORMS:
            r = measure(eng, batch, args.steps, args.warmup, args.repeats, form)
            print(json.dumps({"batch": batch, "prec": "bf16", "form": form, "steps_per_call": args.steps, "repeats": args.repeats, **r}), flush=True)
        for acc, r in measure_kernel(batch, args.steps, args.warmup, args.repeats).items():
            print(json.dumps({"batch": batch, "prec": "bf16", "form": f"jck_feat_match alone, accumulate {acc}", "launches_per_call": args.steps,
                              "repeats": args.repeats, **r}), flush=True)
        del eng
    return 0


if __name__ == "__main__":
    sys.exit(main())
