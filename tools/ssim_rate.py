"""Pairs per second of the SSIM / MS-SSIM pair kernel (jck_ssim_pairs_u8, csrc/ssim.hip) next to the same arithmetic written with torch
on the same device in one run, at the sizes the diversity report is used at: S = 64 / L = 3 and S = 128 / L = 4, P = 4096 random pairs
of 1024 uniform random pictures (seeded).

  kernel      jck_ssim_pairs_u8 into preallocated outputs: one launch, one workgroup per pair, nothing but the pictures read from HBM
  torch       the pictures gathered and converted to fp32 planes, F.conv2d with the separable window (11 x 1, then 1 x 11) on x, y, x x,
              y y, x y, the two maps, their means, F.avg_pool2d for the next level, the combine step - --chunk pairs at a time

Each shape: one untimed call of each path, then --rounds rounds in which the two alternate (a device that is still raising its clocks
favours whoever runs later), each round --calls calls between two device events.  One JSON line per (shape, path, round), then one per
shape with the median seconds per call, pairs per second of both, their ratio (torch / kernel: above 1 the kernel is faster), the bytes
of the pairs' pictures (2 * 3 S^2 each) over the kernel's time as a share of --hbm (the streaming rate the chip reaches, 6.3e12
bytes/s), and the largest difference between the two paths' ssim and ms_ssim.

    timeout -k 10 300 python tools/ssim_rate.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jck-generation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def torch_pairs(x, ia, ib, L, chunk):
    """(ssim [P], ms_ssim [P]) of the definition in fp32 torch on the device"""
    import metrics
    F = torch.nn.functional
    g = torch.as_tensor(metrics._ssim_window(), dtype=torch.float32, device=x.device)
    blur = lambda v: F.conv2d(F.conv2d(v, g.view(1, 1, 11, 1)), g.view(1, 1, 1, 11))
    w = torch.tensor(metrics.MS_SSIM_WEIGHTS[:L], dtype=torch.float32, device=x.device)
    w = w / w.sum()
    ssim, ms = [], []
    for lo in range(0, ia.shape[0], chunk):
        a, b = (x[i[lo:lo + chunk]].permute(0, 3, 1, 2).float().reshape(-1, 1, x.shape[1], x.shape[2]) for i in (ia, ib))      # [p * 3,1,S,S]
        p, factors = a.shape[0] // 3, []
        for l in range(L):
            mx, my = blur(a), blur(b)
            vx, vy, vxy = blur(a * a) - mx * mx, blur(b * b) - my * my, blur(a * b) - mx * my
            cs = (2 * vxy + metrics.SSIM_C2) / (vx + vy + metrics.SSIM_C2)
            ss = (2 * mx * my + metrics.SSIM_C1) / (mx * mx + my * my + metrics.SSIM_C1) * cs
            if l == 0:
                ssim.append(ss.mean(dim=(1, 2, 3)).view(p, 3).mean(dim=1))
            factors.append((ss if l == L - 1 else cs).mean(dim=(1, 2, 3)).clamp_min(0) ** w[l])
            if l + 1 < L:
                a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
        ms.append(torch.stack(factors).prod(dim=0).view(p, 3).mean(dim=1))
    return torch.cat(ssim), torch.cat(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--shapes", nargs="+", default=["64:3", "128:4"], help="S:L")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=512, help="pairs per pass of the torch path")
    ap.add_argument("--hbm", type=float, default=6.3e12)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ssim_rate needs a GPU: a time taken anywhere else says nothing")
    from hipgan._lib import cur_stream, lib
    n, P = args.pictures, args.pairs
    for shape in args.shapes:
        S, L = (int(v) for v in shape.split(":"))
        gen = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randint(0, 256, (n, S, S, 3), device="cuda", generator=gen, dtype=torch.uint8)
        ia = torch.randint(0, n, (P,), device="cuda", generator=gen)
        ib = torch.randint(0, n, (P,), device="cuda", generator=gen)
        ssim, ms = torch.empty(P, device="cuda"), torch.empty(P, device="cuda")
        sq = torch.empty(P, dtype=torch.int64, device="cuda")

        def kernel():
            lib.jck_ssim_pairs_u8(x, n, x, n, S, ia, ib, P, L, ssim, ms, sq, None, cur_stream())

        def by_torch():
            return torch_pairs(x, ia, ib, L, args.chunk)

        paths = {"kernel": kernel, "torch": by_torch}
        kernel()
        t_ssim, t_ms = by_torch()
        torch.cuda.synchronize()
        diff = {"ssim": float((ssim - t_ssim).abs().max()), "ms_ssim": float((ms - t_ms).abs().max())}
        times = {p: [] for p in paths}
        for rnd in range(args.rounds):
            for p, fn in paths.items():
                t = timed(fn, args.calls)
                times[p].append(t)
                print(json.dumps({"shape": shape, "path": p, "round": rnd, "seconds_per_call": t}), flush=True)
        tk, tt = statistics.median(times["kernel"]), statistics.median(times["torch"])
        nbytes = 2.0 * 3 * S * S * P
        print(json.dumps({"shape": shape, "S": S, "L": L, "P": P, "rounds": args.rounds, "calls": args.calls, "kernel_s": tk, "torch_s": tt,
                          "kernel_pairs_per_s": P / tk, "torch_pairs_per_s": P / tt, "torch_over_kernel": tt / tk,
                          "kernel_bytes_per_s": nbytes / tk, "kernel_share_of_hbm": nbytes / tk / args.hbm, "max_difference": diff}), flush=True)
        del x
    return 0


if __name__ == "__main__":
    sys.exit(main())
