"""Which name a launch reports (jck_last_launch) and under which label the profiler books it (jck_prof_collect): one small call
per kernel.  bench.py keys its roofline rows on the labels, and several kernels share one label (the LDS-DMA gather-GEMMs report
the register-staged tile's, the image-side layers carry a <bf16> suffix, the BatchNorm launches have a label and no launch
name), so the pairing is pinned here call by call.  Shapes are the smallest ones tests/test_exact_gpu.py uses to land on each
kernel; the operands are zeros - only the dispatch is looked at, the values are that file's business."""
import ctypes
import os

import pytest
import torch

gpu = pytest.mark.gpu
DT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float32}
PREC_NAME = {0: "bf16", 1: "f32", 2: "bf16x3"}


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def z(n, dtype=torch.float32):
    return torch.zeros(int(n), dtype=dtype, device="cuda")


# the knobs the cases force to 0, and the library's default for each (a JCK_<KEY> preset, read when the library loads, goes before it)
KNOB_DEFAULT = {"igemm_dma_ksplit": 1, "wgrad_ws": 1}


# (op, dims, options, precision, launch name, profiler label); ops and dims as in tests/test_exact_gpu.py's table (upa / g1a:
# jck_conv_up_affine / jck_g1_fwd_affine, shapes of tests/test_sample_eval_gpu.py)
def _p(prec, tile):
    return f"<{PREC_NAME[prec]},{tile}>"


CASES = []
for _prec in (1, 2):          # the register-staged gather-GEMM and weight gradient: the label is the launch name
    CASES += [(op, dims, opt, _prec, "igemm" + _p(_prec, t), "igemm" + _p(_prec, t)) for op, dims, opt, t in (
        ("lin", (768, 256, 256, 8392, 8448, 1, 0), {}, "128,128"), ("down", (1, 4, 64, 128), {"stats": True}, "128,64"),
        ("down", (3, 32, 3, 64), {"stats": True}, "64,128,img"), ("up", (9, 4, 64, 32), {"stats": True}, "64,128"),
        ("up", (5, 4, 128, 3), {"tanh": True}, "16,256"))]
    CASES += [(op, dims, opt, _prec, "wgrad" + _p(_prec, t), "wgrad" + _p(_prec, t)) for op, dims, opt, t in (
        ("wgrad", (7, 8, 64, 128), {}, "128,128"), ("wgrad", (9, 16, 32, 64), {}, "128,64"),
        ("wgrad", (3, 64, 3, 64), {}, "64,64,img"), ("linw", (40, 64, 190, 192, 64, 0, 0), {}, "64,64"))]
CASES += [
    ("lin", (1300, 8392, 8448, 256, 256, 12, 0), {"tune": "igemm_dma_ksplit"}, 0, "igemm<bf16,128,128>", "igemm<bf16,128,128>"),
    ("lin", (300, 8392, 8448, 256, 256, 12, 0), {"tune": "igemm_dma_ksplit"}, 0, "igemm<bf16,128,64>", "igemm<bf16,128,64>"),
    ("down", (3, 16, 3, 32), {"stats": True}, 0, "igemm<bf16,64,128,img>", "igemm<bf16,64,128,img>"),
    ("up", (5, 4, 128, 3), {"tanh": True}, 0, "igemm<bf16,16,256>", "igemm<bf16,16,256>"),
    # the LDS-DMA gather-GEMMs, persistent and not: the label of the register-staged tile of the same size
    ("up", (64, 16, 256, 128), {"stats": True, "group": 64}, 0, "igemm_dma_persist<128,256,8>", "igemm<bf16,128,256>"),
    ("up", (64, 32, 128, 128), {"tanh": True}, 0, "igemm_dma<128,256,3,ws,8>", "igemm<bf16,128,256>"),
    ("down", (256, 16, 128, 256), {}, 0, "igemm_dma_persist<128,128,4>", "igemm<bf16,128,128>"),
    ("down", (4096, 4, 64, 512), {"stats": True}, 0, "igemm_dma<128,128,2>", "igemm<bf16,128,128>"),
    ("down", (1, 4, 64, 128), {"stats": True}, 0, "igemm_dma_persist<128,64,4>", "igemm<bf16,128,64>"),
    ("lin", (21, 500, 512, 250, 256, 1, 1), {}, 0, "igemm_dma<128,64,3,ws>", "igemm<bf16,128,64>"),
    ("up", (9, 4, 64, 32), {"stats": True}, 0, "igemm_dma_persist<64,128,4>", "igemm<bf16,64,128>"),
    ("up", (64, 16, 128, 64), {"tanh": True}, 0, "igemm_dma<64,128,2>", "igemm<bf16,64,128>"),
    ("down", (3, 32, 3, 64), {"stats": True}, 0, "img_down", "img_down<bf16>"),
    ("up", (3, 16, 64, 3), {"tanh": True}, 0, "img_up", "img_up<bf16>"),
    ("wgrad", (7, 8, 64, 128), {}, 0, "wgrad_dma<3,ws>", "wgrad<bf16,128,128>"),
    ("wgrad", (7, 8, 64, 128), {"tune": "wgrad_ws"}, 0, "wgrad_dma<2>", "wgrad<bf16,128,128>"),
    ("wgrad", (5, 8, 32, 192), {}, 0, "wgrad<bf16,128,128>", "wgrad<bf16,128,128>"),
    ("wgrad", (9, 16, 32, 64), {}, 0, "wgrad<bf16,128,64>", "wgrad<bf16,128,64>"),
    ("wgrad", (3, 64, 3, 64), {}, 0, "wgrad<bf16,64,64,img>", "wgrad<bf16,64,64,img>"),
    ("linw", (40, 64, 190, 192, 64, 0, 0), {}, 0, "wgrad<bf16,64,64>", "wgrad<bf16,64,64>"),
    # inference (the Epi::ReluAffine instantiations): the name and label of their tile; Cs = 32 is the gather form of the 16 x 256 tile alone
    ("upa", (1, 4, 64, 32), {}, 0, "igemm_dma<64,128,2>", "igemm<bf16,64,128>"),
    ("upa", (1, 4, 64, 32), {}, 1, "igemm<f32,64,128>", "igemm<f32,64,128>"),
    ("upa", (2, 8, 32, 16), {}, 0, "igemm<bf16,16,256>", "igemm<bf16,16,256>"),
    ("upa", (2, 8, 32, 16), {}, 1, "igemm<f32,16,256>", "igemm<f32,16,256>"),
    ("upa", (2, 8, 32, 16), {}, 2, "igemm<bf16x3,16,256>", "igemm<bf16x3,16,256>"),
    ("g1a", (8, 100, 128, 512), {}, 0, "igemm_dma<128,64,3,ws>", "igemm<bf16,128,64>"),
    ("g1a", (8, 100, 128, 512), {}, 2, "igemm<bf16x3,128,64>", "igemm<bf16x3,128,64>"),
    # BatchNorm (C = 64, 384 rows): a profiler label and no launch name - jck_last_launch keeps what it said before the call
    ("bn_act_fwd", (384, 64), {}, 0, None, "bn_act_fwd"),
    ("bn_act_fwd", (384, 64), {}, 1, None, "bn_act_fwd"),
    ("bn_act_fwd_grouped", (384, 64), {}, 0, None, "bn_act_fwd"),
    ("bn_fwd", (384, 64), {}, 0, None, "bn_act_fwd"),                      # jck_bn_fwd: booked once, whichever form it takes
    ("bn_bwd_res", (384, 64), {}, 0, None, "bn_bwd_resident"),
    ("bn_bwd", (384, 64), {}, 0, None, "bn_bwd_3launch"),                  # two launches: reduce, fused sums + apply
    ("bn_bwd", (384, 64), {}, 1, None, "bn_bwd_3launch"),                  # three launches: reduce, sums, apply
]


def _id(c):
    op, dims, opt, prec, name, label = c
    return f"{name or op}-{PREC_NAME[prec]}" + "".join(f"-{k}" for k in sorted(opt) if k in ("tune",))


def call(G, op, dims, opt, prec):
    L, st, dt = G.lib, G.cur_stream(), DT[prec]
    if op in ("down", "up"):
        if op == "down":
            n, hb, cb, cs = dims
            cbp, oh = L.jck_pad_chan(cb), hb // 2
            x, wp, out = z(n * hb * hb * cbp, dt), z(L.jck_pad_rows(cs) * 16 * cbp, dt), z(n * oh * oh * cs, dt)
            pixels, cstat = n * oh * oh, cs
        else:
            n, hs, cs, cb = dims
            cbp = L.jck_pad_chan(cb)
            x, out = z(n * hs * hs * cs, dt), z(n * 4 * hs * hs * cbp, dt)
            wp = z(16 * 9 * cs if cb <= 4 else 4 * L.jck_pad_rows(cb) * 4 * cs, dt)
            pixels, cstat = n * 4 * hs * hs, cbp
        stats, slots = (z(L.jck_stats_floats(pixels, cstat, 1)), ctypes.c_int(-1)) if opt.get("stats") else (None, None)
        sa = (stats, ctypes.byref(slots) if stats is not None else None)
        if op == "down" and opt.get("group"):
            L.jck_conv_down_grouped(prec, x, wp, out, *sa, n, hb, hb, cb, cs, opt["group"], st)
        elif op == "down":
            L.jck_conv_down(prec, x, wp, out, *sa, n, hb, hb, cb, cs, st)
        elif opt.get("group"):
            L.jck_conv_up_grouped(prec, x, wp, out, *sa, n, hs, hs, cs, cb, opt["group"], st)
        else:
            L.jck_conv_up(prec, x, wp, out, *sa, 1 if opt.get("tanh") else 0, n, hs, hs, cs, cb, st)
    elif op == "upa":
        n, hs, cs, cb = dims
        L.jck_conv_up_affine(prec, z(n * hs * hs * cs, dt), z(4 * L.jck_pad_rows(cb) * 4 * cs, dt), z(cb), z(cb), z(n * 4 * hs * hs * cb, dt),
                             n, hs, hs, cs, cb, st)
    elif op == "g1a":
        b, ci, cip, co = dims
        L.jck_g1_fwd_affine(prec, z(b * cip, dt), z(16 * co * cip, dt), z(co), z(co), z(b * 16 * co, dt), b, cip, co, st)
    elif op == "wgrad":
        n, hb, cb, cs = dims
        oh, ws_bytes = hb // 2, L.jck_conv_wgrad_ws_bytes(n, hb, hb, cb, cs)
        L.jck_conv_wgrad(prec, z(n * oh * oh * cs, dt), z(n * hb * hb * L.jck_pad_chan(cb), dt), z(ws_bytes // 4), ws_bytes,
                         z(cs * cb * 16), 0, n, hb, hb, cb, cs, st)
    elif op == "lin":
        b, k, kp, n, nstore, ks, bias = dims
        L.jck_linear_fwd(prec, z(b * kp, dt), z(L.jck_pad_rows(n) * kp, dt), z(nstore) if bias else None,
                         z(ks * b * nstore, torch.float32 if ks > 1 else dt), b, kp, n, nstore, ks, st)
    elif op == "linw":
        b, n, k, kp, ldgy, pc, phw = dims
        ws_bytes = L.jck_linear_wgrad_ws_bytes(b, kp, n)
        L.jck_linear_wgrad(prec, z(b * ldgy, dt), ldgy, z(b * kp, dt), kp, z(ws_bytes // 4), ws_bytes, z(n * kp), 0, b, n, st)
    else:
        rows, c = dims
        y, a, aux = z(rows * c, dt), z(rows * c, dt), z(4 * c)
        if op == "bn_act_fwd":
            L.jck_bn_act_fwd(prec, y, aux, 0.2, a, rows, c, st)
        elif op == "bn_act_fwd_grouped":
            L.jck_bn_act_fwd_grouped(prec, y, aux, 0.2, a, rows, c, 1, st)
        elif op == "bn_fwd":
            L.jck_bn_fwd(prec, y, z(4 * 2 * c), 4, float(rows), torch.ones(c, device="cuda"), z(c), 1e-5, 0.2, a, aux, None, None, None, None,
                         0.1, rows, c, 1, st)
        else:
            sums, dg, db = z(L.jck_bn_bwd_ws_floats(c)), z(c), z(c)
            if op == "bn_bwd_res":
                sync = torch.zeros(L.jck_grid_sync_bytes() // 4, dtype=torch.int32, device="cuda")
                L.jck_bn_act_bwd_res(prec, a, y, aux, 0.2, sums, z(rows * c, dt), dg, db, rows, c, 1, 1, sync, st)
            else:
                L.jck_bn_act_bwd(prec, a, y, aux, 0.2, sums, z(rows * c, dt), dg, db, rows, c, st)
    torch.cuda.synchronize()


def collect(G):
    cap = 16
    names, cnt, ms, fl = (ctypes.c_char_p * cap)(), (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
    by, sv = (ctypes.c_double * cap)(), (ctypes.c_void_p * cap)()
    n = G.lib.jck_prof_collect(cap, names, cnt, ms, fl, by, sv)
    return [(names[i].decode(), cnt[i]) for i in range(n)]


@gpu
@pytest.mark.parametrize("case", [pytest.param(c, id=_id(c)) for c in CASES])
def test_launch_name_and_profiler_label(G, case):
    op, dims, opt, prec, name, label = case
    knob = opt.get("tune")
    before = G.lib.jck_last_launch().decode()
    collect(G)                                    # drop records an earlier test may have left
    try:
        if knob:
            G.lib.jck_tune(knob.encode(), 0)
        G.lib.jck_prof_enable(1)
        call(G, op, dims, opt, prec)
    finally:
        G.lib.jck_prof_enable(0)
        if knob:
            G.lib.jck_tune(knob.encode(), int(os.environ.get("JCK_" + knob.upper(), KNOB_DEFAULT[knob])))
    got = collect(G)
    assert G.lib.jck_last_launch().decode() == (before if name is None else name), f"{_id(case)}: launch name"
    assert got == [(label, 1)], f"{_id(case)}: the profiler booked {got}, expected one launch under {label}"
