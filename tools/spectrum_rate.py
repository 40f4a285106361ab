"""Rates of the power-spectrum kernel (csrc/spectrum.hip), one JSON line per round and one summary line per size:

  jck_spectrum_u8 at S = 64 and 128, n = 8192 uint8 pictures, luma, no window, with and without the mean plane: pictures per second,
  interleaved round by round with the comparison leg, torch.fft.rfft2 of the same planes ALREADY converted to fp32 on the same device
  (so the comparison pays no conversion, no centring, no power and no bin sums: it is the transform alone)

    timeout -k 10 600 python tools/spectrum_rate.py
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=8192)
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_rate needs a GPU: a time taken anywhere else says nothing")
    from hipgan._lib import cur_stream, lib, load_library
    gen = torch.Generator(device="cuda").manual_seed(0)
    n = args.pictures
    for S in (int(s) for s in args.sizes.split(",")):
        R = load_library().jck_spectrum_bins(S)
        x = torch.randint(0, 256, (n, S, S, 3), device="cuda", generator=gen, dtype=torch.uint8)
        planes = (x.to(torch.float32) * torch.tensor([77.0, 150.0, 29.0], device="cuda") / 256.0).sum(dim=3).contiguous()        # [n][S][S] fp32
        prof = torch.empty(n, R, dtype=torch.float64, device="cuda")
        mean = torch.empty(n, dtype=torch.float64, device="cuda")
        plane2d = torch.empty(S, S, dtype=torch.float64, device="cuda")
        nbytes = load_library().jck_spectrum_ws_bytes(n, S, 1)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        legs = {"profile": lambda: lib.jck_spectrum_u8(x, n, S, 3, None, 1.0, prof, mean, None, None, 0, cur_stream()),
                "profile_mean2d": lambda: lib.jck_spectrum_u8(x, n, S, 3, None, 1.0, prof, mean, plane2d, ws, nbytes, cur_stream()),
                "torch_rfft2": lambda: torch.fft.rfft2(planes)}
        for fn in legs.values():
            fn()
        times = {k: [] for k in legs}
        for rnd in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, args.calls))
                print(json.dumps({"S": S, "leg": k, "round": rnd, "seconds_per_call": times[k][-1]}), flush=True)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"S": S, "pictures": n, "grid": load_library().jck_spectrum_grid(S), **{k + "_s": v for k, v in med.items()},
                          **{k + "_pictures_per_s": n / v for k, v in med.items()}, "profile_over_torch_rfft2": med["profile"] / med["torch_rfft2"],
                          "profile_mean2d_over_torch_rfft2": med["profile_mean2d"] / med["torch_rfft2"]}), flush=True)
        del x, planes, prof, ws
    return 0


if __name__ == "__main__":
    sys.exit(main())
