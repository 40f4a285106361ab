"""Time of a nearest-neighbour index search (metrics.nearest_chunk: jck_knn_index_f32, csrc/knnindex.hip) next to torch on the same
device in one run, at the three shapes the feature is used at:

  pixel64     64 x 50 000 x 12 288   a grid of samples against the training set in pixel space (seeded uint8 data as u8 / 127.5 - 1)
  pixel1000   1 000 x 50 000 x 12 288
  feature     10 000 x 50 000 x 100  generated against real features of the metric network (seeded normal data)

  kernel      the reference walked in chunks of --chunk rows through ref_base / merge, k = --k
  torch       torch.cdist(q, chunk) ** 2, topk(k, smallest) per chunk, the running lists concatenated and cut by topk again - the
              same chunks of the same fp32 matrices (which are staged on the device before anything is timed, for both)

Each shape: one untimed call of each path, then --rounds rounds in which the two alternate (a device that is still raising its clocks
favours whoever runs later), each call between two device events.  One JSON line per (shape, path, round), then one per shape with
the medians, their ratio (torch / kernel: above 1 the kernel is faster) and the achieved fp32 FLOP/s, counting 2 M N D.

    timeout -k 10 300 python tools/neighbour_rate.py
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

SHAPES = {"pixel64": (64, 50000, 12288, "pixel"), "pixel1000": (1000, 50000, 12288, "pixel"), "feature": (10000, 50000, 100, "feature")}


def make(rows, d, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "pixel":
        return torch.randint(0, 256, (rows, d), dtype=torch.uint8, device="cuda", generator=g).to(torch.float32) / 127.5 - 1.0
    return torch.randn(rows, d, device="cuda", generator=g)


def run_kernel(q, ref, k, chunk):
    from metrics import nearest_chunk
    idx = torch.empty(q.shape[0], k, dtype=torch.int64, device="cuda")
    d2 = torch.empty(q.shape[0], k, dtype=torch.float32, device="cuda")
    for lo in range(0, ref.shape[0], chunk):
        nearest_chunk(q, ref[lo:lo + chunk], k, idx, d2, ref_base=lo, merge=lo > 0)
    return idx, d2


def run_torch(q, ref, k, chunk):
    idx = d2 = None
    for lo in range(0, ref.shape[0], chunk):
        d = torch.cdist(q, ref[lo:lo + chunk]) ** 2
        v, i = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
        i = i + lo
        if idx is not None:
            v, pick = torch.topk(torch.cat([d2, v], 1), k, dim=1, largest=False)
            i = torch.gather(torch.cat([idx, i], 1), 1, pick)
        idx, d2 = i, v
    return idx, d2


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=sorted(SHAPES), default=["pixel64", "pixel1000", "feature"])
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    ref_cache = {}
    for name in args.shapes:
        m, n, d, kind = SHAPES[name]
        if (n, d, kind) not in ref_cache:
            ref_cache.clear()
            ref_cache[(n, d, kind)] = make(n, d, kind, 0)
        ref, q = ref_cache[(n, d, kind)], make(m, d, kind, 1)
        paths = {"kernel": lambda: run_kernel(q, ref, args.k, args.chunk), "torch": lambda: run_torch(q, ref, args.k, args.chunk)}
        first = {p: fn() for p, fn in paths.items()}                          # the warm-up of this shape, and a look at the answers
        torch.cuda.synchronize()
        agree = float((first["kernel"][0][:, 0] == first["torch"][0][:, 0]).float().mean())
        times = {p: [] for p in paths}
        for rnd in range(args.rounds):
            for p, fn in paths.items():
                t, _ = timed(fn)
                times[p].append(t)
                print(json.dumps({"shape": name, "path": p, "round": rnd, "seconds": t}), flush=True)
        tk, tt = statistics.median(times["kernel"]), statistics.median(times["torch"])
        print(json.dumps({"shape": name, "M": m, "N": n, "D": d, "k": args.k, "chunk": args.chunk, "rounds": args.rounds,
                          "kernel_s": tk, "torch_s": tt, "torch_over_kernel": tt / tk, "kernel_flops": 2.0 * m * n * d / tk,
                          "torch_flops": 2.0 * m * n * d / tt, "nearest_index_agreement": agree}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
