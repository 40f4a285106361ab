"""Makes tests/golden/resize_any_u8.json: what Pillow's bilinear resize - the call behind transforms.Resize((S, S)) on a PIL image -
returns for seeded inputs of any size, square or not, up- and downscaled, for both engine sizes.  Run where Pillow is installed:
    python tests/golden/make_golden_resize_any.py
Inputs are regenerated from the seeds by the tests (`inputs`, `case_inputs`: no Pillow needed for those); the fixture holds digests,
64 sampled pixels per case and the full output of the two smallest cases."""
import base64
import hashlib
import json
import os
import zlib

import numpy as np

# (source height, source width, output side, images): both engine sizes; identity on one or both axes; 3, 5, 7, 9 and 11 taps;
# clamped borders; several bands of output rows per image; non-square sources
CASES = ((32, 32, 64, 4), (8, 8, 64, 4), (48, 48, 64, 4), (64, 64, 64, 4), (96, 96, 64, 4), (100, 75, 64, 4), (218, 178, 64, 4),
         (64, 300, 64, 4), (1, 1, 64, 4), (5, 7, 64, 4), (37, 50, 128, 4), (130, 130, 128, 4), (256, 256, 128, 4), (512, 512, 64, 2))
FULL = ((1, 1, 64), (5, 7, 64))             # the two smallest: every output byte is in the fixture


def case_name(h, w, s):
    return f"{h}x{w}_to_{s}"


def case_seed(h, w, s):
    return 1000 * h + 7 * w + s


def inputs(seed, n, h, w):
    """make_golden_resize.inputs for an h x w source: seeded noise, with image 0 saturated, 1 a horizontal ramp, 2 a checkerboard"""
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 256, size=(n, 3, h, w)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    x[0] = 255                                                        # saturated
    if n > 1:
        x[1] = ((xx * 255) // max(w - 1, 1)).astype(np.uint8)         # horizontal ramp
    if n > 2:
        x[2] = (((xx + yy) % 2) * 255).astype(np.uint8)               # checkerboard (worst case for the rounding)
    return x


def case_inputs(h, w, s, n):
    return inputs(case_seed(h, w, s), n, h, w)


def sample_points(h, w, s, n):
    rs = np.random.RandomState(99 + case_seed(h, w, s))
    pts = [(int(rs.randint(n)), int(rs.randint(3)), int(rs.randint(s)), int(rs.randint(s))) for _ in range(60)]
    return pts + [(n - 1, 0, 0, 0), (n - 1, 1, s - 1, s - 1), (n - 1, 2, 0, s - 1), (n - 1, 0, s - 1, 0)]


def pack_full(y):
    """every byte of an output, C order, zlib-compressed and base64-encoded (a JSON list of them would be 30 times the size)"""
    return base64.b64encode(zlib.compress(np.ascontiguousarray(y).tobytes(), 9)).decode("ascii")


def unpack_full(text, shape):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype=np.uint8).reshape(shape)


def pil_resize(chw, size):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0)))
    return np.asarray(im.resize((size, size), Image.BILINEAR)).transpose(2, 0, 1)


def main():
    import PIL
    out = {"pillow": PIL.__version__, "cases": {}}
    for h, w, s, n in CASES:
        x = case_inputs(h, w, s, n)
        y = np.ascontiguousarray(np.stack([pil_resize(img, s) for img in x]))
        case = {"h": h, "w": w, "s": s, "n": n, "seed": case_seed(h, w, s), "sha256": hashlib.sha256(y.tobytes()).hexdigest(),
                "sum": int(y.astype(np.int64).sum()), "samples": [[*p, int(y[p])] for p in sample_points(h, w, s, n)]}
        if (h, w, s) in FULL:
            case["full_zlib_b64"] = pack_full(y)
        out["cases"][case_name(h, w, s)] = case
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resize_any_u8.json")
    with open(path, "w") as f:                      # one case per line
        rows = ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in out["cases"].items())
        f.write(f'{{"pillow":{json.dumps(out["pillow"])},"cases":{{\n{rows}\n}}}}\n')
    print("wrote", path)


if __name__ == "__main__":
    main()
