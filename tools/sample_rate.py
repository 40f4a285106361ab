"""Images per second of generator sampling (batch 256, bf16, 64x64 by default), three ways on the same device in one run:

  train       DcganEngine.sample(z): train-mode BatchNorm, the training schedule's forward (11 launches)
  fused       DcganEngine.sample(z, bn="running"): eval-mode BatchNorm folded into the products' epilogues (8 launches)
  two_launch  the same eval-mode arithmetic as product + jck_bn_act_fwd on the running aux table, built here from the per-op
              entry points (12 launches) - the form the fused epilogue replaces; it exists in this script only

Each path: `--warmup` calls, then `--repeats` groups of `--calls` calls timed with device events around the group (the launches
of a group queue back to back, so host enqueue time is hidden as in use).  Reported: the median group's rate and the spread
(min, max) over the groups, and per call the device time next to the host's enqueue time: a path whose two times meet is
bound by the host, and its rate says nothing about its kernels.  One JSON line per path.

    timeout -k 10 120 python tools/sample_rate.py --path train && timeout -k 10 120 python tools/sample_rate.py --path fused && \\
    timeout -k 10 120 python tools/sample_rate.py --path two_launch
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jck-generation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def two_launch_sampler(eng, batch):
    """eval-mode G forward from the per-op ABI: every stage a product and a separate BatchNorm + ReLU pass over its output"""
    import ctypes

    from hipgan._lib import cur_stream, lib
    prec, dt, dev = eng.prec, torch.bfloat16, eng.device
    sd = {k: v.to(dev).float().contiguous() for k, v in eng.state_dicts()[0].items()}
    nconv = sum(1 for k in sd if k.startswith("conv"))
    ns = nconv - 1                                                   # BatchNorm stages
    c1 = sd["conv1.weight"].shape[1]
    zp = torch.zeros(batch, 128, dtype=dt, device=dev)
    w1 = torch.empty(16 * c1 * 128, dtype=dt, device=dev)
    lib.jck_pack_g1(prec, sd["conv1.weight"], 100, c1, 128, w1, cur_stream())
    ups = []
    for i in range(2, nconv + 1):
        w = sd[f"conv{i}.weight"]
        cs, cb = w.shape[0], w.shape[1]
        rows = 16 if cb <= 4 else lib.jck_pad_rows(cb)
        wp = torch.empty((16 * 9 * cs) if cb <= 4 else (4 * rows * 4 * cs), dtype=dt, device=dev)
        lib.jck_pack_up(prec, w, cs, cb, wp, cur_stream())
        ups.append((wp, cs, cb))
    chans = [c1 >> i for i in range(ns)]
    aux = [torch.empty(4 * c, device=dev) for c in chans]
    y = [torch.empty(batch, 4 << i, 4 << i, c, dtype=dt, device=dev) for i, c in enumerate(chans)]
    a = [torch.empty_like(t) for t in y]
    img = torch.empty(batch, eng.size, eng.size, 4, dtype=dt, device=dev)
    out = torch.empty(batch, 3, eng.size, eng.size, device=dev)
    arr = lambda ts: (ctypes.c_void_p * ns)(*[t.data_ptr() for t in ts])
    tabs = [arr([sd[f"norm{i + 1}.{k}"] for i in range(ns)]) for k in ("weight", "bias", "running_mean", "running_var")]
    auxp, cc = arr(aux), (ctypes.c_int * ns)(*chans)

    def run(z):
        st = cur_stream()
        zp[:, :100] = z
        lib.jck_bn_eval_aux(ns, *tabs, auxp, cc, 1e-5, st)
        lib.jck_g1_fwd(prec, zp, w1, y[0], None, None, batch, 128, c1, st)
        for i in range(ns):
            h = 4 << i
            lib.jck_bn_act_fwd(prec, y[i], aux[i], 0.0, a[i], batch * h * h, chans[i], st)
            wp, cs, cb = ups[i]
            lib.jck_conv_up(prec, a[i], wp, y[i + 1] if i < ns - 1 else img, None, None, 0 if i < ns - 1 else 1, batch, h, h, cs, cb, st)
        lib.jck_nhwc4_to_nchw(prec, img, out, batch, eng.size * eng.size, st)
        return out
    return run


def measure(fn, batch, warmup, calls, repeats):
    """host_ms: what the host needs to ENQUEUE a call (the clock stops before the device is waited for); where it comes close to
    device_ms the group measures the host and not the kernels"""
    import time
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    rates, host, dev = [], [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        rates.append(batch * calls / (ms * 1e-3))
        host.append((t1 - t0) * 1e3 / calls)
        dev.append(ms / calls)
    rates.sort(), host.sort(), dev.sort()
    m = len(rates) // 2
    return {"images_per_s": round(rates[m], 1), "min": round(rates[0], 1), "max": round(rates[-1], 1),
            "device_ms_per_call": round(dev[m], 4), "host_enqueue_ms_per_call": round(host[m], 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["train", "fused", "two_launch", "all"], default="all")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import GanOracle
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    eng = DcganEngine(batch=args.batch, prec="bf16")
    eng.load_state(orc.g, orc.d)
    z = torch.randn(args.batch, 100, generator=torch.Generator().manual_seed(0)).cuda()
    for _ in range(3):                       # running statistics off their initial (0, 1)
        eng.sample(z)
    paths = {"train": lambda: eng.sample(z), "fused": lambda: eng.sample(z, bn="running")}
    if args.path in ("two_launch", "all"):
        run2 = two_launch_sampler(eng, args.batch)
        ref, got = eng.sample(z, bn="running"), run2(z)
        # the same arithmetic up to the rounding of y between the two launches: a bf16 ulp per stage
        assert float((ref - got).abs().max()) < 0.1, "the two-launch eval form disagrees with the fused one"
        paths["two_launch"] = lambda: run2(z)
    for name in (["train", "fused", "two_launch"] if args.path == "all" else [args.path]):
        r = measure(paths[name], args.batch, args.warmup, args.calls, args.repeats)
        print(json.dumps({"path": name, "batch": args.batch, "prec": "bf16", "calls": args.calls, "repeats": args.repeats, **r}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
