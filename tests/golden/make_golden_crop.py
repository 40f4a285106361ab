"""Makes tests/golden/crop_resize_u8.json: what Pillow returns for PIL.Image.crop((x0, y0, x0 + Wc, y0 + Hc)).resize((S, S), BILINEAR)
- CenterCrop / RandomCrop in front of transforms.Resize((S, S)) on a PIL image; the resize of the cropped array, not resize(box=...) -
for seeded inputs.  Run where Pillow is installed:
    python tests/golden/make_golden_crop.py
Inputs are those of make_golden_resize_any.inputs, regenerated from the seeds by the tests (no Pillow needed for those); the fixture
holds digests, a sum and 60 sampled bytes per case and every byte of the two smallest cases."""
import hashlib
import json
import os

import numpy as np

from make_golden_resize_any import inputs, pack_full

# (source height, source width, box height, box width, y0, x0, output side, images): the face-set crop; centred crops of odd
# differences; a box that ends on the image's last byte; an identity axis; the CIFAR crop; one pixel; a box narrower than a dword;
# a non-square box; a large source
CASES = ((218, 178, 178, 178, 20, 0, 64, 4), (100, 75, 75, 75, 12, 0, 64, 4), (37, 50, 37, 37, 0, 6, 128, 4), (48, 48, 41, 41, 7, 7, 64, 4),
         (64, 300, 64, 64, 0, 118, 64, 4), (32, 32, 28, 28, 3, 1, 64, 4), (5, 7, 1, 1, 4, 6, 64, 4), (5, 7, 3, 2, 1, 5, 64, 4),
         (100, 75, 90, 33, 10, 41, 128, 4), (512, 512, 500, 500, 5, 9, 64, 2))
CENTRED = ((218, 178, 178, 178, 20, 0, 64), (100, 75, 75, 75, 12, 0, 64), (37, 50, 37, 37, 0, 6, 128), (64, 300, 64, 64, 0, 118, 64))   # `center` origins
FULL = ((5, 7, 1, 1, 4, 6, 64), (5, 7, 3, 2, 1, 5, 64))             # the two smallest: every output byte is in the fixture


def case_name(hs, ws, hc, wc, y0, x0, s):
    return f"{hs}x{ws}_box_{hc}x{wc}_at_{y0}_{x0}_to_{s}"


def case_seed(hs, ws, hc, wc, y0, x0, s):
    return 1000 * hs + 7 * ws + s + 31 * hc + 3 * wc + 5 * y0 + x0


def case_inputs(hs, ws, hc, wc, y0, x0, s, n):
    return inputs(case_seed(hs, ws, hc, wc, y0, x0, s), n, hs, ws)


def sample_points(case, n):
    s = case[6]
    rs = np.random.RandomState(77 + case_seed(*case))
    return [(int(rs.randint(n)), int(rs.randint(3)), int(rs.randint(s)), int(rs.randint(s))) for _ in range(60)]


def pil_crop_resize(chw, hc, wc, y0, x0, size):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0)))
    return np.asarray(im.crop((x0, y0, x0 + wc, y0 + hc)).resize((size, size), Image.BILINEAR)).transpose(2, 0, 1)


def main():
    import PIL
    cases = {}
    for *case, n in CASES:
        hs, ws, hc, wc, y0, x0, s = case
        x = case_inputs(*case, n)
        y = np.ascontiguousarray(np.stack([pil_crop_resize(img, hc, wc, y0, x0, s) for img in x]))
        rec = {"hs": hs, "ws": ws, "hc": hc, "wc": wc, "y0": y0, "x0": x0, "s": s, "n": n, "seed": case_seed(*case),
               "sha256": hashlib.sha256(y.tobytes()).hexdigest(), "sum": int(y.astype(np.int64).sum()),
               "samples": [[*p, int(y[p])] for p in sample_points(tuple(case), n)]}
        if tuple(case) in FULL:
            rec["full_zlib_b64"] = pack_full(y)
        cases[case_name(*case)] = rec
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "crop_resize_u8.json")
    with open(path, "w") as f:                      # one case per line
        rows = ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in cases.items())
        f.write(f'{{"pillow":{json.dumps(PIL.__version__)},"cases":{{\n{rows}\n}}}}\n')
    print("wrote", path)


if __name__ == "__main__":
    main()
