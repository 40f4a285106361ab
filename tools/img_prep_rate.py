"""Time of the input transform of the training step - gather by index, Resize, ToTensor, Normalize, instance-noise mix into NHWC4 -
for the 2x kernel (img_prep_u8_kernel, csrc/ew.hpp), the any-size kernel (img_prep_u8_any_kernel, csrc/resize.hpp) and the box kernel
beside it (img_prep_u8_box_kernel: the same code with a box's corner added to its addresses) in one run:

  old   32x32 -> 64    B 256   jck_img_prep_u8_rng                      (what a CIFAR run launches)
  any   32x32 -> 64    B 256   jck_img_prep_u8_any, the same batch
  any   64x64 -> 64, 218x178 -> 64 at B 256; 128x128 -> 128, 256x256 -> 128 at B 128
  box   whole-image boxes at 32x32 -> 64, 218x178 -> 64, 256x256 -> 128: the same work as `any` at those shapes
  box   the crops themselves: the centred 178x178 of 218x178 -> 64, the centred 28x28 of 32x32 -> 64

bf16 NHWC4 output with the in-kernel noise, as the step runs them; the batch is a random index vector into a seeded uint8 dataset
of --images images.  Every path: untimed launches first, then --rounds rounds in which the paths alternate, each round's call
`reps` back-to-back launches between two device events, reps chosen so that a call lasts about --window seconds.  One JSON line per
path with the median time per launch, the bytes the algorithm must move (the batch's source bytes once plus the output) and the
bandwidth that makes.  Then the DCGAN step at batch 256 (bf16) fed from a 64x64 dataset beside the same step fed from a 32x32 one, and
fed from a 218x178 dataset squeezed beside the same dataset's centred 178x178 box, alternating in blocks of --steps steps.

    timeout -k 10 300 python tools/img_prep_rate.py
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

#        name            kernel  Hs   Ws   S    B    box (Hc, Wc, y0, x0) of the box kernel
PATHS = (("old_32_64", "old", 32, 32, 64, 256, None), ("any_32_64", "any", 32, 32, 64, 256, None), ("any_64_64", "any", 64, 64, 64, 256, None),
         ("any_218x178_64", "any", 218, 178, 64, 256, None), ("any_128_128", "any", 128, 128, 128, 128, None),
         ("any_256_128", "any", 256, 256, 128, 128, None),
         ("box_32_64", "box", 32, 32, 64, 256, (32, 32, 0, 0)), ("box_218x178_64", "box", 218, 178, 64, 256, (218, 178, 0, 0)),
         ("box_256_128", "box", 256, 256, 128, 128, (256, 256, 0, 0)),
         ("box_178sq_of_218x178_64", "box", 218, 178, 64, 256, (178, 178, 20, 0)), ("box_28sq_of_32_64", "box", 32, 32, 64, 256, (28, 28, 2, 2)))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def kernel_paths(images):
    from hipgan import PREC_BF16, lib
    from hipgan._lib import cur_stream
    from hipgan.engine import resize_taps
    gen = torch.Generator(device="cuda").manual_seed(1)
    rng = torch.tensor([2024, 0, 1, 0], dtype=torch.int32, device="cuda")
    data, out = {}, {}
    for name, kind, hs, ws, s, b, box in PATHS:
        if (hs, ws) not in data:
            data[(hs, ws)] = torch.randint(0, 256, (images, 3, hs, ws), dtype=torch.uint8, device="cuda", generator=gen)
        if (b, s) not in out:
            out[(b, s)] = torch.empty(b, s, s, 4, dtype=torch.bfloat16, device="cuda")
    idx = {b: torch.randint(0, images, (b,), device="cuda", generator=gen) for b in (128, 256)}
    fns = {}
    for name, kind, hs, ws, s, b, box in PATHS:
        d, o, i = data[(hs, ws)], out[(b, s)], idx[b]
        if kind == "old":
            fns[name] = lambda d=d, o=o, i=i, b=b: lib.jck_img_prep_u8_rng(PREC_BF16, d, i, rng, 0, 0.9, 0.1, o, b, 32, 32, cur_stream())
        elif kind == "box":
            hc, wc, y0, x0 = box
            t = resize_taps(hc, wc, s, "cuda")
            fns[name] = lambda d=d, o=o, i=i, b=b, hs=hs, ws=ws, s=s, t=t, hc=hc, wc=wc, y0=y0, x0=x0: lib.jck_img_prep_u8_box(
                PREC_BF16, d, i, None, None, None, rng, 0, 0.9, 0.1, o, None, b, hs, ws, hc, wc, y0, x0, s, t, cur_stream())
        else:
            t = resize_taps(hs, ws, s, "cuda")
            fns[name] = lambda d=d, o=o, i=i, b=b, hs=hs, ws=ws, s=s, t=t: lib.jck_img_prep_u8_any(
                PREC_BF16, d, i, None, None, rng, 0, 0.9, 0.1, o, None, b, hs, ws, s, t, cur_stream())
    return fns


def step_paths(images):
    from hipgan.engine import DcganEngine, DeviceBatch
    from model import DCGAN
    B = 256
    gen = torch.Generator(device="cuda").manual_seed(2)
    fns, datasets = {}, {}
    for name, shape, box in (("step_32_data", (32, 32), None), ("step_64_data", (64, 64), None), ("step_218x178_squeezed", (218, 178), None),
                             ("step_218x178_center", (218, 178), (178, 178, (20, 0)))):
        eng = DcganEngine(batch=B, prec="bf16")
        torch.manual_seed(12345)
        g, d = DCGAN.Generator(), DCGAN.Discriminator()
        g.apply(DCGAN.weights_init)
        d.apply(DCGAN.weights_init)
        eng.load_state(g.state_dict(), d.state_dict())
        if shape not in datasets:
            datasets[shape] = torch.randint(0, 256, (images, 3, *shape), dtype=torch.uint8, device="cuda", generator=gen)
        data = datasets[shape]
        batches = [DeviceBatch(data, torch.randint(0, images, (B,), device="cuda", generator=gen), box=box) for _ in range(4)]
        count = [0]

        def one(eng=eng, batches=batches, count=count):
            i = count[0]
            count[0] += 1
            eng.step_async(batches[i % 4], None, 2e-4, next_real=batches[(i + 1) % 4])
        fns[name] = one
    return fns


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096, help="images of each seeded dataset")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per timed call")
    ap.add_argument("--steps", type=int, default=40, help="engine steps per timed block (0: skip the step timing)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("img_prep_rate: needs a GPU (a time measured elsewhere says nothing about it)")
    fns = kernel_paths(args.images)
    reps = {}
    for name, fn in fns.items():                      # warm-up, and the launches a window takes
        timed(fn, 20)
        reps[name] = max(20, int(args.window / timed(fn, 50)))
    times = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, reps[name]))
    for name, kind, hs, ws, s, b, box in PATHS:
        t = statistics.median(times[name])
        nbytes = b * (3 * (box[0] * box[1] if box else hs * ws) + s * s * 4 * 2)
        print(json.dumps({"path": name, "B": b, "source": [hs, ws], **({"box": list(box)} if box else {}), "size": s, "launches_per_call": reps[name], "rounds": args.rounds,
                          "us": t * 1e6, "us_min": min(times[name]) * 1e6, "us_max": max(times[name]) * 1e6, "bytes": nbytes,
                          "GBps": nbytes / t * 1e-9}), flush=True)
    if args.steps > 0:
        steps = step_paths(args.images)
        for fn in steps.values():
            timed(fn, 10)
        st = {name: [] for name in steps}
        for _ in range(args.rounds):
            for name, fn in steps.items():
                st[name].append(timed(fn, args.steps))
        for name in steps:
            print(json.dumps({"path": name, "B": 256, "prec": "bf16", "steps_per_call": args.steps, "rounds": args.rounds,
                              "ms": statistics.median(st[name]) * 1e3, "ms_min": min(st[name]) * 1e3, "ms_max": max(st[name]) * 1e3}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
