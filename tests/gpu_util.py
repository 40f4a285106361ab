"""Helpers for the GPU parity tests: NCHW fp32 (CPU, PyTorch layout) <-> NHWC T (device, library layout)."""
import torch

from hipgan import PREC_BF16, PREC_F32, lib  # noqa: F401
from hipgan._lib import cur_stream  # noqa: F401

DT = {PREC_BF16: torch.bfloat16, PREC_F32: torch.float32}
# relative-to-max tolerances per precision: F32 = exact fp32 MFMA (summation order only), BF16 = bf16 storage (2^-9)
TOL = {PREC_F32: 3e-6, PREC_BF16: 1.5e-2}


def to_nhwc(x_nchw, prec, cpad=None):
    """CPU NCHW fp32 -> device NHWC of the library's element type, channels zero-padded to cpad."""
    n, c, h, w = x_nchw.shape
    cp = cpad or (4 if c == 3 else c)
    t = torch.zeros(n, h, w, cp, dtype=torch.float32)
    t[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return t.to(DT[prec]).cuda().contiguous()


def from_nhwc(t, c=None):
    """device NHWC -> CPU NCHW fp32 (first c channels)."""
    t = t.float().cpu()
    if c is not None:
        t = t[..., :c]
    return t.permute(0, 3, 1, 2).contiguous()


def rnd(x, prec):
    """Round a CPU fp32 tensor the way the library stores it (bf16 in fast mode)."""
    return x.to(torch.bfloat16).float() if prec == PREC_BF16 else x


def pack_down(w, prec):
    cs, cb = w.shape[0], w.shape[1]
    wp = torch.empty(lib.jck_pad_rows(cs) * 16 * lib.jck_pad_chan(cb), dtype=DT[prec], device="cuda")
    lib.jck_pack_down(prec, w.cuda().contiguous(), cs, cb, wp, cur_stream())
    return wp


def pack_up(w, prec):
    cs, cb = w.shape[0], w.shape[1]
    wp = torch.empty(4 * lib.jck_pad_rows(cb) * 4 * cs, dtype=DT[prec], device="cuda")
    lib.jck_pack_up(prec, w.cuda().contiguous(), cs, cb, wp, cur_stream())
    return wp


def stats_buf(pixels, c, nyrep=1):
    import ctypes
    return torch.full((lib.jck_stats_floats(pixels, c, nyrep),), float("nan"), device="cuda"), ctypes.c_int(0)


def stats_sum(buf, slots, c):
    """[slots][2][C] partials -> (sum[C], sumsq[C]) on the CPU."""
    v = buf[:slots.value * 2 * c].view(slots.value, 2, c).double().sum(0).float().cpu()
    return v[0], v[1]


def check(got, ref, tol, what=""):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs()
    m = err.max().item()
    if not (m <= tol * scale):
        idx = torch.nonzero(err == err.max())[0].tolist()
        nbad = int((err > tol * scale).sum())
        raise AssertionError(f"{what}: max err {m:.3e} > {tol:.1e} * {scale:.3e}; {nbad}/{err.numel()} bad; first worst at {idx}: "
                             f"got {got[tuple(idx)].item():.6g} ref {ref[tuple(idx)].item():.6g}; "
                             f"rel-l2 {((got-ref).norm()/ref.norm()).item():.3e}")
    return m / scale


def make_checkpoints(d):
    """Writes plain.pt (no average), ema.pt (an average whose weights differ from the live ones) and cgan.pt into directory d, each
    from a fresh batch-8 engine with the oracle's weights -> (plain, ema, cgan) paths."""
    import os
    from hipgan.engine import CganEngine, DcganEngine
    from oracle.gan_oracle import GanOracle
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    eng = DcganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gen = torch.Generator().manual_seed(9)
    for _ in range(30):          # running statistics that belong to the weights (the initial (0, 1) give a flat grey image in eval mode)
        eng.sample(torch.randn(8, 100, generator=gen))
    g, dd = eng.state_dicts()
    plain, both, cgan = (os.path.join(str(d), f) for f in ("plain.pt", "ema.pt", "cgan.pt"))
    torch.save({"model_g": g, "model_d": dd}, plain)
    co = GanOracle("cgan", lr=2e-4, seed=12345)
    ce = CganEngine(batch=8, prec="bf16")
    ce.load_state(co.g, co.d)
    for _ in range(30):
        ce.sample(torch.randn(8, 100, generator=gen), torch.nn.functional.one_hot(torch.randint(0, 100, (8,), generator=gen), 100))
    cg, cd = ce.state_dicts()
    torch.save({"model_g": cg, "model_d": cd}, cgan)
    ema = {k: (v * 0.5 if k.endswith("conv3.weight") else v.clone()) for k, v in g.items()}
    torch.save({"model_g": g, "model_d": dd, "model_g_ema": ema}, both)
    return plain, both, cgan
