"""Time of the per-cluster sums of a Lloyd iteration (jck_segment_mean_f32, csrc/cluster.hip) next to torch on the same device in one
run, at the sizes the mode-coverage clustering is used at: N = 50 000 rows of D = 15 360 (grid 4) and 3 840 (grid 2) discriminator
features, K = 100 and 1 000 clusters, labels uniform over the clusters (seeded).

  kernel      jck_segment_mean_f32 into preallocated sum / count / centre and workspace: five launches, no float atomics
  torch       sum.zero_().index_add_(0, labels, x) and torch.bincount(labels, minlength=K): float atomics, bits that change from run to run

Each shape: one untimed call of each path, then --rounds rounds in which the two alternate (a device that is still raising its clocks
favours whoever runs later), each round --calls calls between two device events.  One JSON line per (shape, path, round), then one per
shape with the median seconds per call, their ratio (torch / kernel: above 1 the kernel is faster), the bytes of x over the time and
that rate as a share of --hbm (the streaming rate the chip reaches, 6.3e12 bytes/s), and the largest difference between the two sums
relative to the largest sum (they add in different orders).

    timeout -k 10 300 python tools/cluster_rate.py
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
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--widths", type=int, nargs="+", default=[15360, 3840])
    ap.add_argument("--clusters", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.3e12)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cluster_rate needs a GPU: a time taken anywhere else says nothing")
    from hipgan._lib import cur_stream, lib, load_library
    n = args.rows
    for d in args.widths:
        x = torch.randn(n, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        for k in args.clusters:
            labels = torch.randint(0, k, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            total, centre = torch.empty(k, d, device="cuda"), torch.zeros(k, d, device="cuda")
            count = torch.empty(k, dtype=torch.int32, device="cuda")
            ws_bytes = load_library().jck_segment_ws_bytes(n, d, k)
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device="cuda")
            t_sum = torch.empty(k, d, device="cuda")

            def kernel():
                lib.jck_segment_mean_f32(x, n, d, labels, k, total, count, centre, ws, cur_stream())

            def by_torch():
                t_sum.zero_().index_add_(0, labels, x)
                return torch.bincount(labels, minlength=k)

            paths = {"kernel": kernel, "torch": by_torch}
            kernel()
            t_count = by_torch()
            torch.cuda.synchronize()
            assert torch.equal(count.long(), t_count)
            diff = float((total - t_sum).abs().max() / t_sum.abs().max())
            shape = f"{n}x{d}/k{k}"
            times = {p: [] for p in paths}
            for rnd in range(args.rounds):
                for p, fn in paths.items():
                    t = timed(fn, args.calls)
                    times[p].append(t)
                    print(json.dumps({"shape": shape, "path": p, "round": rnd, "seconds_per_call": t}), flush=True)
            tk, tt = statistics.median(times["kernel"]), statistics.median(times["torch"])
            nbytes = 4.0 * n * d
            print(json.dumps({"shape": shape, "N": n, "D": d, "K": k, "rounds": args.rounds, "calls": args.calls, "kernel_s": tk, "torch_s": tt,
                              "torch_over_kernel": tt / tk, "kernel_bytes_per_s": nbytes / tk, "torch_bytes_per_s": nbytes / tt,
                              "kernel_share_of_hbm": nbytes / tk / args.hbm, "torch_share_of_hbm": nbytes / tt / args.hbm,
                              "workspace_bytes": ws_bytes, "max_rel_difference": diff}), flush=True)
            del total, centre, ws, t_sum
        del x
    return 0


if __name__ == "__main__":
    sys.exit(main())
