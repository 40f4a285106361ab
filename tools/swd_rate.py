"""Rates of the sliced-Wasserstein kernels (csrc/swd.hip), one JSON line per round and one summary line per leg:

  project   jck_swd_project_u8 at S = 64, three levels, P = 128 patches, D = 128 directions: pictures per second (and the fp32
            multiply-adds of the [P x 147] . [147 x D] products per second), with jck_swd_patch_stats_u8 beside it
  sort      jck_sort_rows_f32 of 128 rows of M = 2^20 standard normal keys: keys per second, interleaved round by round with
            torch.sort(dim=1) of the same tensor (the comparison leg) and checked against it
  swd       the whole metrics.swd at n = 8192, S = 64 (defaults: 3 levels, 128 patches, 128 directions, 4 repeats): seconds

    timeout -k 10 600 python tools/swd_rate.py
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--pictures", type=int, default=2048, help="pictures of the projection leg")
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--num", type=int, default=8192, help="pictures a set of the whole-metric leg (0: skip it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("swd_rate needs a GPU: a time taken anywhere else says nothing")
    import metrics
    from hipgan import swd as H
    from hipgan._lib import cur_stream, lib, load_library
    gen = torch.Generator(device="cuda").manual_seed(0)

    n, S, L, P, D = args.pictures, 64, 3, 128, 128
    x = torch.randint(0, 256, (n, S, S, 3), device="cuda", generator=gen, dtype=torch.uint8)
    pos, dirs = H.draw(n, S, L, P, D, 1, 0)
    pos_t, dirs_t = torch.from_numpy(pos).cuda(), torch.from_numpy(dirs[0]).cuda()
    mean, rstd = torch.zeros(L, 3, device="cuda"), torch.full((L, 3), 0.05, device="cuda")
    proj = torch.empty(L * D, n * P, device="cuda")
    part = torch.empty(n, L, 3, 2, dtype=torch.float64, device="cuda")
    s1, s2 = torch.empty(L, 3, dtype=torch.float64, device="cuda"), torch.empty(L, 3, dtype=torch.float64, device="cuda")
    legs = {"project": lambda: lib.jck_swd_project_u8(x, n, S, L, pos_t, P, dirs_t, D, mean, rstd, proj, n * P, cur_stream()),
            "stats": lambda: lib.jck_swd_patch_stats_u8(x, n, S, L, pos_t, P, part, s1, s2, cur_stream())}
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for rnd in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.calls))
            print(json.dumps({"leg": k, "round": rnd, "seconds_per_call": times[k][-1]}), flush=True)
    tp, ts = statistics.median(times["project"]), statistics.median(times["stats"])
    print(json.dumps({"leg": "project", "S": S, "L": L, "P": P, "D": D, "pictures": n, "project_s": tp, "project_pictures_per_s": n / tp,
                      "project_fma_per_s": n * L * P * 147 * D / tp, "stats_s": ts, "stats_pictures_per_s": n / ts}), flush=True)
    del x, proj, part

    rows, M = args.rows, args.keys
    keys = torch.randn(rows, M, device="cuda", generator=gen)
    out = torch.empty_like(keys)
    nbytes = load_library().jck_sort_rows_ws_bytes(rows, M)
    ws = torch.empty(max(nbytes // 4, 1), device="cuda")
    legs = {"own": lambda: lib.jck_sort_rows_f32(keys, rows, M, out, ws, nbytes, cur_stream()), "torch": lambda: torch.sort(keys, dim=1)}
    legs["own"]()
    same = bool(torch.equal(out, torch.sort(keys, dim=1).values))
    times = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.calls))
            print(json.dumps({"leg": "sort", "path": k, "round": rnd, "seconds_per_call": times[k][-1]}), flush=True)
    to, tt = statistics.median(times["own"]), statistics.median(times["torch"])
    print(json.dumps({"leg": "sort", "rows": rows, "M": M, "tile": load_library().jck_sort_rows_tile(), "own_s": to, "torch_s": tt, "own_keys_per_s": rows * M / to,
                      "torch_keys_per_s": rows * M / tt, "own_over_torch": to / tt, "equal_to_torch": same}), flush=True)
    del keys, out, ws

    if args.num:
        n = args.num
        a = torch.randint(0, 256, (n, S, S, 3), device="cuda", generator=gen, dtype=torch.uint8)
        b = torch.randint(0, 256, (n, S, S, 3), device="cuda", generator=gen, dtype=torch.uint8)
        secs = []
        for rnd in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = metrics.swd(a, b)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            print(json.dumps({"leg": "swd", "round": rnd, "seconds": secs[-1]}), flush=True)
        print(json.dumps({"leg": "swd", "n": n, "S": S, "levels": 3, "patches": 128, "dirs": 128, "repeats": 4, "seconds": min(secs), "swd": [float(v) for v in r["swd"]]}),
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
