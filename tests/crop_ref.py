"""Shared by tests/test_crop_cpu.py and tests/test_crop_gpu.py: the Pillow fixture tests/golden/crop_resize_u8.json, its seeded inputs,
and each case's full expected output - computed once per process by the host statement of the transform (resize_pil_u8 of the cropped
slice) and accepted only if its digest is the fixture's, i.e. Pillow's bytes."""
import functools
import json
import os

import torch

from resize_any_ref import HERE, check, normalized  # noqa: F401  (puts tests/golden on sys.path)
from make_golden_crop import CASES, CENTRED, case_inputs, case_name  # noqa: E402  (input generator only: numpy, no Pillow)


@functools.lru_cache(maxsize=None)
def gold():
    return json.load(open(os.path.join(HERE, "golden", "crop_resize_u8.json")))


def ids():
    return [case_name(*c[:7]) for c in CASES]


def host_crop_resize(x, hc, wc, y0, x0, s):
    """uint8 [..., Hs, Ws] numpy -> uint8 [..., s, s] numpy: the host statement of the transform on the slice"""
    from preprocess.dcgan_data_preprocessor import resize_pil_u8
    return resize_pil_u8(torch.from_numpy(x[..., y0:y0 + hc, x0:x0 + wc].copy()), s).numpy()


@functools.lru_cache(maxsize=None)
def reference(hs, ws, hc, wc, y0, x0, s, n):
    """(inputs uint8 [n,3,hs,ws], Pillow's output uint8 [n,3,s,s] for the case's box) as read-only numpy arrays"""
    x = case_inputs(hs, ws, hc, wc, y0, x0, s, n)
    y = host_crop_resize(x, hc, wc, y0, x0, s)
    check(y, gold()["cases"][case_name(hs, ws, hc, wc, y0, x0, s)])
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y
