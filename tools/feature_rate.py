"""Images per second of discriminator feature extraction (bf16, 64x64; batch 64 and 256 by default) beside scoring, on the same
device in one run, by the protocol of tools/score_rate.py (tools/sample_rate.py: measure):

  score     jck_engine_score
  features  jck_engine_features(grid, max): the same conv stack, one jck_grid_pool per stage in the head's place
  pool      those jck_grid_pool launches alone, on activations of the stages' shapes: bytes moved (the activations read once, the
            feature rows written once) over device time, to hold against the device's HBM bandwidth

`--warmup` calls, then `--repeats` groups of `--calls` calls between device events; the median group's rate and the spread; the
paths alternate over `--rounds`.  One JSON line per (path, batch, round).

    timeout -k 10 180 python tools/feature_rate.py
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


def main(argv=None):
    from sample_rate import measure
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="measurements of each path, the paths alternating")
    args = ap.parse_args(argv)
    from hipgan._lib import cur_stream, lib
    from hipgan.engine import DcganEngine
    from hipgan.probe import feature_layout
    from model import DCGAN
    torch.manual_seed(12345)
    g_state, d_state = DCGAN.Generator().state_dict(), DCGAN.Discriminator().state_dict()      # fresh modules: the rate does not depend on the weights
    layout, F = feature_layout(64, args.grid)
    for batch in args.batches:
        eng = DcganEngine(batch=batch, prec="bf16")
        eng.load_state(g_state, d_state)
        img = (torch.rand(batch, 3, 64, 64, generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
        logit, prob = torch.empty(batch, device="cuda"), torch.empty(batch, device="cuda")
        feat = torch.empty(batch, F, device="cuda")
        acts = [torch.randn(batch, h, h, c, device="cuda").to(torch.bfloat16) for _, _, c, h in layout]
        nbytes = sum(a.numel() * 2 for a in acts) + feat.numel() * 4

        def score():
            lib.jck_engine_score(eng._h, img, None, None, batch, logit, prob, cur_stream())

        def features():
            lib.jck_engine_features(eng._h, img, batch, args.grid, 0, feat, F, cur_stream())

        def pool():
            for a, (_, col0, c, h) in zip(acts, layout):
                lib.jck_grid_pool(eng.prec, a, batch, h, c, args.grid, 0, feat, F, col0, cur_stream())

        paths = {"score": score, "features": features, "pool": pool}
        for rnd in range(args.rounds):
            for name, fn in paths.items():
                r = measure(fn, batch, args.warmup, args.calls, args.repeats)
                if name == "pool":
                    r["bytes_per_call"] = nbytes
                    r["gb_per_s"] = round(nbytes / (r["device_ms_per_call"] * 1e-3) / 1e9, 1)
                print(json.dumps({"path": name, "batch": batch, "round": rnd, "prec": "bf16", "grid": args.grid, "calls": args.calls,
                                  "repeats": args.repeats, **r}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
