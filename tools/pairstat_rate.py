"""Time of the pairwise-statistics entry points (csrc/pairstat.hip) at the shapes the evaluation branch calls them at (50 000 real and
10 000 generated feature rows of width 100, seeded normal data):

  poly3_rr     jck_poly3_sum_f64   50 000 x 50 000 x 100, skip_diag     the real x real term of KID
  poly3_fr     jck_poly3_sum_f64   10 000 x 50 000 x 100                the cross term
  knn_r        jck_knn_radius2_f32 50 000 x 100, k = 3                  the real manifold's radii
  hit_fr       jck_manifold_hit_u8 10 000 queries x 50 000 references   precision
  hit_rf       jck_manifold_hit_u8 50 000 queries x 10 000 references   recall

Each shape: one untimed call, then --rounds calls, each between two device events.  One JSON line per (shape, round), then one per
shape with the median, the spread (largest minus smallest round) and the achieved fp32 FLOP/s, counting 2 M N D (the hit kernel
leaves its walk early, so its figure is a lower bound of its rate).  To compare two builds, run this once per library (JCKGAN_LIB
names the other one), alternating, in fresh processes.

    timeout -k 10 120 python tools/pairstat_rate.py
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

N_REAL, N_FAKE, D, K = 50000, 10000, 100, 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def main(argv=None):
    from hipgan._lib import cur_stream, lib, load_library
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    g = torch.Generator(device="cuda").manual_seed(0)
    real = torch.randn(N_REAL, D, device="cuda", generator=g)
    fake = 0.8 * torch.randn(N_FAKE, D, device="cuda", generator=g) + 0.3
    out = torch.empty(1, dtype=torch.float64, device="cuda")
    ws = torch.empty(load_library().jck_pairstat_ws_bytes(N_REAL, N_REAL) // 8, dtype=torch.float64, device="cuda")
    r2 = {"r": torch.empty(N_REAL, device="cuda"), "f": torch.empty(N_FAKE, device="cuda")}
    hit = torch.empty(N_REAL, dtype=torch.uint8, device="cuda")
    lib.jck_knn_radius2_f32(fake, N_FAKE, D, K, r2["f"], cur_stream())
    shapes = {
        "poly3_rr": (N_REAL, N_REAL, lambda: lib.jck_poly3_sum_f64(real, N_REAL, real, N_REAL, D, 1.0 / D, 1.0, 1, out, ws, cur_stream())),
        "poly3_fr": (N_FAKE, N_REAL, lambda: lib.jck_poly3_sum_f64(fake, N_FAKE, real, N_REAL, D, 1.0 / D, 1.0, 0, out, ws, cur_stream())),
        "knn_r": (N_REAL, N_REAL, lambda: lib.jck_knn_radius2_f32(real, N_REAL, D, K, r2["r"], cur_stream())),
        "hit_fr": (N_FAKE, N_REAL, lambda: lib.jck_manifold_hit_u8(fake, N_FAKE, real, r2["r"], N_REAL, D, hit, cur_stream())),
        "hit_rf": (N_REAL, N_FAKE, lambda: lib.jck_manifold_hit_u8(real, N_REAL, fake, r2["f"], N_FAKE, D, hit, cur_stream())),
    }
    for name, (m, n, fn) in shapes.items():
        fn()                                                                 # the warm-up of this shape (knn_r also fills hit_fr's radii)
        torch.cuda.synchronize()
        times = []
        for rnd in range(args.rounds):
            t, _ = timed(fn)
            times.append(t)
            print(json.dumps({"shape": name, "round": rnd, "seconds": t}), flush=True)
        med = statistics.median(times)
        print(json.dumps({"shape": name, "M": m, "N": n, "D": D, "rounds": args.rounds, "median_s": med, "spread_s": max(times) - min(times),
                          "flops": 2.0 * m * n * D / med}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
