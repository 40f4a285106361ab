"""Shared by tests/test_resize_any_cpu.py and tests/test_resize_any_gpu.py: the Pillow fixture tests/golden/resize_any_u8.json, its
seeded inputs, and each case's full expected output - computed once per process by the host statement of the transform
(preprocess.dcgan_data_preprocessor.resize_pil_u8) and accepted only if its digest is the fixture's, i.e. Pillow's bytes."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_resize_any import CASES, case_inputs, case_name, unpack_full  # noqa: E402  (input generator only: numpy, no Pillow)

HDR = 8                                  # include/jckgan.h: header words of a tap table
MAGIC = 0x7a736572


@functools.lru_cache(maxsize=None)
def gold():
    return json.load(open(os.path.join(HERE, "golden", "resize_any_u8.json")))


def check(y, case):
    """y uint8 [n,3,S,S] against one fixture case: digest, sum, the full output where recorded, the sampled pixels"""
    y = np.ascontiguousarray(y)
    assert y.dtype == np.uint8 and y.shape == (case["n"], 3, case["s"], case["s"])
    for n, c, yy, xx, v in case["samples"]:
        assert int(y[n, c, yy, xx]) == v, (n, c, yy, xx, int(y[n, c, yy, xx]), v)
    if "full_zlib_b64" in case:
        assert np.array_equal(y, unpack_full(case["full_zlib_b64"], y.shape))
    assert int(y.astype(np.int64).sum()) == case["sum"]
    assert hashlib.sha256(y.tobytes()).hexdigest() == case["sha256"]


@functools.lru_cache(maxsize=None)
def reference(h, w, s, n):
    """(inputs uint8 [n,3,h,w], Pillow's output uint8 [n,3,s,s]) as read-only numpy arrays"""
    from preprocess.dcgan_data_preprocessor import resize_pil_u8
    x = case_inputs(h, w, s, n)
    y = resize_pil_u8(torch.from_numpy(x), s).numpy()
    check(y, gold()["cases"][case_name(h, w, s)])
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def normalized(u8):
    """ToTensor + Normalize(0.5, 0.5) in the kernels' fp32 operation order"""
    return (torch.from_numpy(np.array(u8)).float() / 255.0 - 0.5) / 0.5


def taps_table(h, w, s):
    """jck_resize_taps_build(h, w, s) as an int32 numpy array (host call, no GPU)"""
    from hipgan.engine import resize_taps_host
    return resize_taps_host(h, w, s).numpy()


def split_table(t, s):
    """-> ((lo, cnt, k[K][s]) of the x axis, the same of the y axis) after checking the header"""
    assert int(t[0]) == MAGIC and int(t[3]) == s and tuple(t[6:8]) == (0, 0)
    kx, ky = int(t[4]), int(t[5])
    assert t.size == HDR + s * (2 + kx) + s * (2 + ky)
    ax, ay = t[HDR:HDR + s * (2 + kx)], t[HDR + s * (2 + kx):]
    return (ax[:s], ax[s:2 * s], ax[2 * s:].reshape(kx, s)), (ay[:s], ay[s:2 * s], ay[2 * s:].reshape(ky, s))


def apply_taps(x, t, s):
    """The two rounded passes of the transform in numpy, from a tap table: x uint8 [n,3,h,w] -> uint8 [n,3,s,s]"""
    def axis(a, lo, cnt, k):                     # along the last axis
        length = a.shape[-1]
        assert lo.min() >= 0 and cnt.min() >= 1 and (lo + cnt).max() <= length and cnt.max() <= k.shape[0]
        acc = np.full(a.shape[:-1] + (s,), 1 << 21, dtype=np.int64)
        for j in range(k.shape[0]):
            assert not k[j][cnt <= j].any() and k[j].min() >= 0           # nothing past an output's last tap, nothing negative
            acc += k[j].astype(np.int64) * a[..., np.minimum(lo + j, length - 1)]
        assert acc.max() < 2 ** 31                                          # the sum fits 32 bits
        return np.clip(acc >> 22, 0, 255)
    (xlo, xcnt, xk), (ylo, ycnt, yk) = split_table(t, s)
    hp = axis(x.astype(np.int64), xlo, xcnt, xk)
    return axis(hp.swapaxes(-1, -2), ylo, ycnt, yk).swapaxes(-1, -2).astype(np.uint8)
