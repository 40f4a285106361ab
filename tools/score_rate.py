"""Images per second of discriminator scoring (bf16, 64x64; batch 64 and 256 by default), three ways on the same device in one run:

  engine      jck_engine_score as shipped (in bf16: the two_launch form, which this script measured to be the faster one)
  fused       eval-mode BatchNorm + LeakyReLU folded into the Conv2d products' epilogues: jck_conv_down_affine per stage, built here
              from the per-op entry points (7 launches for a DCGAN: input transform, fold, 4 stages, head)
  two_launch  the same eval-mode arithmetic as jck_conv_down + jck_bn_act_fwd on the same eval aux tables, from the per-op entry
              points as well (11 launches)

Each path: `--warmup` calls, then `--repeats` groups of `--calls` calls timed with device events around the group (the launches
of a group queue back to back, so host enqueue time is hidden as in use).  Reported: the median group's rate and the spread
(min, max) over the groups, and per call the device time next to the host's enqueue time: a path whose two times meet is
bound by the host, and its rate says nothing about its kernels.  The paths are measured `--rounds` times each, alternating, so
that none always runs on the cooler or the slower-clocked device.  One JSON line per (path, batch, round).

    timeout -k 10 180 python tools/score_rate.py
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jck-generation_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def per_op_scorer(eng, batch, fused):
    """eval-mode D forward from the per-op ABI: every stage ONE launch with the affine and the LeakyReLU in its epilogue (fused), or a
    product and a separate BatchNorm + LeakyReLU pass over its output"""
    import ctypes

    from hipgan._lib import cur_stream, lib
    prec, dt, dev = eng.prec, torch.bfloat16, eng.device
    sd = {k: v.to(dev).float().contiguous() for k, v in eng.state_dicts()[1].items()}
    ns = sum(1 for k in sd if k.startswith("norm") and k.endswith(".weight"))
    downs = []
    for i in range(1, ns + 1):
        w = sd[f"conv{i}.weight"]
        cs, cb = w.shape[0], w.shape[1]
        wp = torch.empty(lib.jck_pad_rows(cs) * 16 * lib.jck_pad_chan(cb), dtype=dt, device=dev)
        lib.jck_pack_down(prec, w, cs, cb, wp, cur_stream())
        downs.append((wp, cs, cb))
    chans = [d[1] for d in downs]
    c5 = sd[f"conv{ns + 1}.weight"].shape[1]
    head = torch.empty(16 * c5, device=dev)
    lib.jck_pack_head(sd[f"conv{ns + 1}.weight"], c5, head, cur_stream())
    aux = [torch.empty(4 * c, device=dev) for c in chans]
    x = torch.empty(batch, eng.size, eng.size, 4, dtype=dt, device=dev)
    y = [torch.empty(batch, eng.size >> (i + 1), eng.size >> (i + 1), c, dtype=dt, device=dev) for i, c in enumerate(chans)]
    a = [torch.empty_like(t) for t in y]
    logit, prob = torch.empty(batch, device=dev), torch.empty(batch, device=dev)
    arr = lambda ts: (ctypes.c_void_p * ns)(*[t.data_ptr() for t in ts])
    tabs = [arr([sd[f"norm{i + 1}.{k}"] for i in range(ns)]) for k in ("weight", "bias", "running_mean", "running_var")]
    auxp, cc = arr(aux), (ctypes.c_int * ns)(*chans)

    def run(img):
        st = cur_stream()
        lib.jck_img_prep(prec, img, None, 1.0, 0.0, x, batch, eng.size * eng.size, st)
        lib.jck_bn_eval_aux(ns, *tabs, auxp, cc, 1e-5, st)
        h = x
        for i in range(ns):
            hb = eng.size >> i
            wp, cs, cb = downs[i]
            if fused:
                lib.jck_conv_down_affine(prec, h, wp, aux[i][:cs], aux[i][cs:2 * cs], 0.2, a[i], batch, hb, hb, cb, cs, st)
            else:
                lib.jck_conv_down(prec, h, wp, y[i], None, None, batch, hb, hb, cb, cs, st)
                lib.jck_bn_act_fwd(prec, y[i], aux[i], 0.2, a[i], batch * (hb // 2) * (hb // 2), cs, st)
            h = a[i]
        lib.jck_score_head(prec, h, head, None, batch, 16 * c5, logit, prob, st)
        return logit
    return run


def main(argv=None):
    from sample_rate import measure
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["engine", "fused", "two_launch", "all"], default="all")
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="measurements of each path, the paths alternating")
    args = ap.parse_args(argv)
    from hipgan._lib import cur_stream, lib
    from hipgan.engine import DcganEngine
    from model import DCGAN
    torch.manual_seed(12345)
    g_state, d_state = DCGAN.Generator().state_dict(), DCGAN.Discriminator().state_dict()      # fresh modules: the rate does not depend on the weights
    for batch in args.batches:
        eng = DcganEngine(batch=batch, prec="bf16")
        eng.load_state(g_state, d_state)
        img = (torch.rand(batch, 3, 64, 64, generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
        logit, prob = torch.empty(batch, device="cuda"), torch.empty(batch, device="cuda")

        def engine():
            lib.jck_engine_score(eng._h, img, None, None, batch, logit, prob, cur_stream())
            return logit
        paths = {"engine": engine}
        ref = engine().clone()
        for name, fused in (("fused", True), ("two_launch", False)):
            if args.path in (name, "all"):
                run = per_op_scorer(eng, batch, fused)
                got = run(img).clone()
                # the same arithmetic up to the rounding of y between the two launches: a bf16 ulp per stage
                assert float((ref - got).abs().max()) < 0.05 * max(1.0, float(ref.abs().max())), f"the {name} form disagrees with the engine"
                paths[name] = lambda run=run: run(img)
        for rnd in range(args.rounds):          # the paths alternate: a device that is still raising its clocks favours whoever runs later
            for name in (["engine", "fused", "two_launch"] if args.path == "all" else [args.path]):
                r = measure(paths[name], batch, args.warmup, args.calls, args.repeats)
                print(json.dumps({"path": name, "batch": batch, "round": rnd, "prec": "bf16", "calls": args.calls, "repeats": args.repeats, **r}),
                      flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
