"""CPU references of the image-side elementwise kernels of csrc/ew.hpp (img_prep, axpy_noise, interp, nhwc4_to_nchw, tanh_bwd,
gp_norm, gp_grad, img_prep_u8), in float64 torch from the storage-rounded inputs, and the seeded inputs that
tests/test_image_ew_ref_cpu.py and tests/test_image_ew_gpu.py share.

Bit-for-bit references of fp32 arithmetic formed in fp64: a product of two fp32 values has 48 significant bits and is exact in fp64, so
rn(a * b) is fp64-multiply-then-round; a sum of two fp32 values is either exact in fp64 or (exponents more than 29 apart) lies beside
the larger operand, far from every fp32 midpoint, so rn(a + b) is fp64-add-then-round as well.  An fma, rn(a * b + c), is the one
operation whose fp64 sum can be inexact AND lie beside an fp32 midpoint; there the second rounding may go the other way.
fma_is_unambiguous says where that cannot happen, and the tests assert it for every element of their inputs - a condition on the inputs
(change the seed if it fails), never on the kernel.

candidates_* return (forms, fma_sums): forms maps the name of every fp32 result a legal contraction of the kernel's expression can
give to that result (fp32 tensor); fma_sums maps the name of each fma in them to (its fp64 sum, a mask of the elements at which that
sum is exact in fp64)."""
import functools
import math

import numpy as np
import torch

PREC_BF16, PREC_F32, PREC_BF16X3 = 0, 1, 2
DT = {PREC_BF16: torch.bfloat16, PREC_F32: torch.float32, PREC_BF16X3: torch.float32}
GRID_CAP = 8192 * 256                               # ew_grid: at most 8192 workgroups of 256 threads, one item each per trip
# (N, HW) of every per-pixel kernel: the smallest launch; HW odd (image boundaries inside a wave); the shape of test_ops_gpu.py;
# 2,100,003 pixels (past the cap, both image boundaries inside a workgroup, the first in the first trip); past the cap, one image
SHAPES = [(1, 1), (5, 37), (3, 4096), (3, 700_001), (1, 2_097_152 + 259)]
GP_NORM_CASES = [(3, 1), (3, 255), (3, 256), (3, 257), (3, 4096), (3, 16384), (300, 64)]        # (N, per_image4)
U8_SHAPES = [(1, 1), (1, 7), (6, 1), (5, 9), (32, 32)]                                            # (Hs, Ws)
U8_IDX = [3, 0, 3, 1]                               # a repeat and an unused image out of 5
KEEP, MIX = 0.9, 0.1                                # the instance-noise mix of the step


def f32(v):
    """the fp32 value a C float argument takes, as a Python float"""
    return float(np.float32(v))


def rnd(x, prec):
    """gpu_util.rnd: a CPU fp32 tensor rounded the way the library stores it"""
    return x.to(torch.bfloat16).float() if prec == PREC_BF16 else x


def rn(x64):
    """fp64 -> the nearest fp32 (ties to even), kept as fp64"""
    return x64.float().double()


def store(x32, prec):
    """rn_T: an fp32 result as the kernel stores it (f2bf rounds to nearest even; NaN stays NaN)"""
    return x32.to(DT[prec])


def bits(t):
    """the bit patterns of an fp32 or bf16 tensor"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _fma(a, b, c):
    """rn(a * b + c) of fp32 values held in fp64 -> (fp64 sum, mask: the fp64 sum is exact).  TwoSum (Knuth): the rounding error of
    an fp64 addition is itself an fp64 number and is recovered exactly by six additions."""
    p = a * b                                       # exact: 24 x 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    return s, err == 0


def fma_is_unambiguous(e64, exact=None):
    """True where rounding the fp64 sum e64 of an fma to fp32 gives the correctly rounded fp32 result whatever the fp64 rounding
    did: e64 is not within 2^-50 relative of the midpoint of two neighbouring fp32 values (the fp64 rounding moved the exact sum by
    at most 2^-53 relative, so it stayed on its side of the midpoint), or e64 is an fp32 value itself, or - where the caller knows it,
    `exact` - the fp64 sum is the exact sum, rounded once."""
    f = e64.float()
    d = f.double()
    toward = torch.where(e64 > d, math.inf, -math.inf).float()
    other = torch.nextafter(f, toward).double()
    mid = 0.5 * d + 0.5 * other                     # exact (halving first: no overflow at the top of the range)
    near = (e64 != d) & ((e64 - mid).abs() <= 2.0 ** -50 * e64.abs())
    ok = ~near | ~torch.isfinite(e64) | ~torch.isfinite(d)
    return ok if exact is None else ok | exact


def ambiguous_count(fma_sums):
    """number of elements at which some fma of the candidates is ambiguous"""
    return sum(int((~fma_is_unambiguous(e, ex)).sum()) for e, ex in fma_sums.values())


# ---- the contractable expressions -------------------------------------------------------------------------------------------------
def candidates_axpy(keep, mix, x, nz):
    """keep * x + mix * nz  (axpy_noise_kernel: `r = keep * v; r += mix * noise`; img_prep_kernel and img_prep_u8_kernel pin form A)
       A: fma(mix, nz, rn(keep * x))     B: rn(rn(keep * x) + rn(mix * nz))     C: fma(keep, x, rn(mix * nz))"""
    keep, mix, x, nz = f32(keep), f32(mix), x.double(), nz.double()
    kx, mn = rn(keep * x), rn(mix * nz)
    a, a_ex = _fma(torch.full_like(nz, mix), nz, kx)
    c, c_ex = _fma(torch.full_like(x, keep), x, mn)
    forms = {"A": a.float(), "B": (kx + mn).float(), "C": c.float()}
    return forms, {"A": (a, a_ex), "C": (c, c_ex)}


def candidates_interp(al, a, b):
    """al * a + (1 - al) * b with t = rn(1 - al)  (interp_kernel, and the xhat half of axpy_noise_kernel)
       U: rn(rn(al * a) + rn(t * b))     Fa: fma(al, a, rn(t * b))     Fb: fma(t, b, rn(al * a))"""
    al, a, b = al.double(), a.double(), b.double()
    t = rn(1.0 - al)                                # a sum of two fp32 values
    pa, pb = rn(al * a), rn(t * b)
    fa, fa_ex = _fma(al, a, pb)
    fb, fb_ex = _fma(t, b, pa)
    forms = {"U": (pa + pb).float(), "Fa": fa.float(), "Fb": fb.float()}
    return forms, {"Fa": (fa, fa_ex), "Fb": (fb, fb_ex)}


def candidates_tanh_bwd(scale, g, y):
    """scale * g * (1 - y * y) = rn(rn(scale * g) * w)     U: w = rn(1 - rn(y * y))     F: w = fma(-y, y, 1)"""
    scale, g, y = f32(scale), g.double(), y.double()
    q = rn(scale * g)
    wf, wf_ex = _fma(-y, y, torch.ones_like(y))
    forms = {"U": (q * rn(1.0 - rn(y * y))).float(), "F": (q * rn(wf)).float()}
    return forms, {"F": (wf, wf_ex)}


def candidates_gp_grad(coef, nr, v):
    """f = nr > 0 ? rn(rn(coef * rn(nr - 1)) / nr) : 0, then rn(v * f): one form, nothing in it can fuse (a product of a difference, a
    quotient, a product).  The fp32 quotient of two fp32 values is fp64-divide-then-round (53 >= 2 * 24 + 2 bits).  A NaN norm fails
    `nr > 0` and gives f = 0, as the kernel does today."""
    coef, nr, v = f32(coef), nr.double(), v.double()
    f = torch.where(nr > 0, rn(rn(coef * rn(nr - 1.0)) / nr), torch.zeros_like(nr))
    return {"one": (v * f).float()}, {}


# ---- jck_img_prep_u8 --------------------------------------------------------------------------------------------------------------
def _up2_last(a):
    """Pillow's bilinear 2x along the last axis on int32: out[2k] = (a[k-1] + 3 a[k] + 2) >> 2, out[2k+1] = (3 a[k] + a[k+1] + 2) >> 2,
    the taps clamped at the borders"""
    n = a.shape[-1]
    k = torch.arange(n)
    am, ap = a[..., (k - 1).clamp(min=0)], a[..., (k + 1).clamp(max=n - 1)]
    return torch.stack([(am + 3 * a + 2) >> 2, (3 * a + ap + 2) >> 2], dim=-1).flatten(-2)


def up2_pil_u8(data_u8, idx=None):
    """[Ntot, 3, Hs, Ws] uint8 (-> gathered by idx) -> [B, 3, 2Hs, 2Ws] uint8: the horizontal pass, then the vertical pass, each
    rounded to uint8 (img_prep_u8_kernel's integer part)"""
    a = (data_u8 if idx is None else data_u8[torch.as_tensor(idx, dtype=torch.int64)]).to(torch.int32)
    h = _up2_last(a)
    return _up2_last(h.transpose(-1, -2)).transpose(-1, -2).contiguous().to(torch.uint8)


def up2_pil_ref(data_u8, idx=None):
    """-> [B, 3, 2Hs, 2Ws] fp32: ToTensor and Normalize(0.5, 0.5) of up2_pil_u8 in the kernel's fp32 operations, (u8 / 255 - 0.5) / 0.5"""
    return (up2_pil_u8(data_u8, idx).float() / 255.0 - 0.5) / 0.5


# ---- gp_norm ----------------------------------------------------------------------------------------------------------------------
def gp_norm_bound(per_image4):
    """Relative bound on gp_norm_kernel's fp32 norm against the fp64 norm of the same stored values.  Every term of the sum is
    non-negative, so the sum's relative error is at most the number of roundings a term can pass through: a thread adds
    ceil(P / 256) groups of at most 5 operations (four squares summed and added to the running sum), then 6 wave levels (four row
    rotations, two levels over the four rows) and the 3 additions of the four waves' sums: k = 5 ceil(P / 256) + 9.  The square root
    halves a relative error and adds one rounding of its own: (k / 2 + 1) * 2^-24."""
    k = 5 * ((per_image4 + 255) // 256) + 9
    return (k / 2 + 1) * 2.0 ** -24


def gp_norm_sim(g):
    """gp_norm_kernel's summation order in numpy fp32, every operation rounded on its own (no fused multiply-add): g [P, 4] fp32 ->
    the fp32 norm.  The rotations' direction is immaterial to the bound."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    p = g.shape[0]
    pad = np.zeros(((p + 255) // 256 * 256, 4), np.float32)
    pad[:p] = g
    sq = pad * pad
    q = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
    s = np.zeros(256, np.float32)
    for j in range(pad.shape[0] // 256):
        s = s + q[j * 256:(j + 1) * 256]            # thread t adds its groups t, t + 256, ...
    v = s.reshape(4, 4, 16)                         # wave, row, lane
    for n in (8, 4, 2, 1):
        v = v + np.roll(v, n, axis=-1)
    r = v[:, :, 0]
    w = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    return np.sqrt(((w[0] + w[1]) + w[2]) + w[3], dtype=np.float32)


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------
# One seed per (kernel, case, precision).  A case whose inputs turn out ambiguous (test_image_ew_ref_cpu.py) gets another seed here -
# the threshold of fma_is_unambiguous never moves.
_KERNEL_ID = {"img_prep": 1, "axpy": 2, "interp": 3, "tanh_bwd": 4, "gp_grad": 5, "gp_norm": 6, "u8": 7, "nhwc4": 8, "mix_interp": 9}
RESEED = {}


def seed_of(kernel, case, prec):
    key = (kernel, case, prec)
    return RESEED.get(key, 100_000 * _KERNEL_ID[kernel] + 10 * (hash_case(case) % 9973) + prec)


def hash_case(case):
    """a stable small integer of a tuple of integers (Python's hash of a tuple of ints is stable too, but this says what it is)"""
    h = 0
    for v in case:
        h = (h * 1_000_003 + int(v)) % 2_147_483_647
    return h


def _gen(kernel, case, prec):
    return torch.Generator().manual_seed(seed_of(kernel, case, prec))


def make_img_prep(n, hw):
    """-> img [N, 3, HW] fp32 in [-1, 1), noise [N, 3, HW] fp32 normal (fp32 inputs in every precision)"""
    g = _gen("img_prep", (n, hw), PREC_F32)
    return torch.rand(n, 3, hw, generator=g) * 2 - 1, torch.randn(n, 3, hw, generator=g)


def make_axpy(n, hw, prec):
    """-> x [N, HW, 4] stored values, lane 3 NaN (the kernel assigns lane 3, it does not carry it), noise [N, 3, HW] fp32"""
    g = _gen("axpy", (n, hw), prec)
    x = rnd(torch.randn(n, hw, 4, generator=g), prec)
    x[..., 3] = math.nan
    return x, torch.randn(n, 3, hw, generator=g)


def make_interp(n, hw, prec):
    """-> a, b [N, HW, 4] stored values (all four lanes: the kernel interpolates lane 3 like the others), alpha [N] in [0, 1)"""
    g = _gen("interp", (n, hw), prec)
    return rnd(torch.randn(n, hw, 4, generator=g), prec), rnd(torch.randn(n, hw, 4, generator=g), prec), torch.rand(n, generator=g)


def make_tanh_bwd(n, hw, prec):
    """-> g, y = tanh(normal) [N, HW, 4] stored values"""
    g = _gen("tanh_bwd", (n, hw), prec)
    return rnd(torch.randn(n, hw, 4, generator=g), prec), rnd(torch.tanh(torch.randn(n, hw, 4, generator=g)), prec)


def make_tanh_special(prec):
    """-> g, y [64]: y = 1, -1, 0, -0; in fp32 then +-(1 - 2^-24) and 1 - 2^-12 + k 2^-24, |k| <= 20 (around where the two forms of
    1 - y * y differ most); in bf16 the values beside 1 and beside 0; the rest 0.5"""
    gen = torch.Generator().manual_seed(seed_of("tanh_bwd", (64,), prec))
    g = rnd(torch.randn(64, generator=gen), prec)
    ys = [1.0, -1.0, 0.0, -0.0]
    if prec == PREC_F32:
        ys += [1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24)] + [1.0 - 2.0 ** -12 + k * 2.0 ** -24 for k in range(-20, 21)]
    else:
        ys += [1.0 - 2.0 ** -8, 1.0 - 2.0 ** -7, 2.0 ** -8]
    y = torch.tensor((ys + [0.5] * 64)[:64])
    assert torch.equal(rnd(y, prec), y)
    return g, y


def make_gp_grad(n, hw, prec):
    """-> g [N, HW, 4] stored values, norms [N] fp32 in [0.25, 2.25), all different (not the norms of g: the kernel takes them as
    given); with N = 5 image 3 has norm 0"""
    g = _gen("gp_grad", (n, hw), prec)
    v = rnd(torch.randn(n, hw, 4, generator=g) * 0.02, prec)
    nr = torch.rand(n, generator=g) * 2 + 0.25
    if n == 5:
        nr[3] = 0.0
    return v, nr


def make_gp_norm(n, p, prec):
    """-> g [N, P, 4] stored values (all four lanes count), image 1 all zero"""
    g = _gen("gp_norm", (n, p), prec)
    v = rnd(torch.randn(n, p, 4, generator=g) * 0.02, prec)
    v[1] = 0.0
    return v


def make_u8(hs, ws):
    """-> data [5, 3, Hs, Ws] uint8 (image 0 saturated, image 1 a 0 / 255 checkerboard - the worst case of the rounding), noise
    [4, 3, 2Hs, 2Ws] fp32"""
    g = _gen("u8", (hs, ws), PREC_F32)
    data = torch.randint(0, 256, (5, 3, hs, ws), generator=g, dtype=torch.int32).to(torch.uint8)
    data[0] = 255
    yy, xx = torch.meshgrid(torch.arange(hs), torch.arange(ws), indexing="ij")
    data[1] = (((xx + yy) % 2) * 255).to(torch.uint8)
    return data, torch.randn(4, 3, 2 * hs, 2 * ws, generator=g)


def nchw_as_pixels(t):
    """[N, 3, HW] -> [N, HW, 3]"""
    return t.permute(0, 2, 1).contiguous()


def expected_img_prep(keep, mix, img, noise):
    """img_prep_kernel / img_prep_u8_kernel: form A of candidates_axpy on [N, 3, HW] (noise None: rn(keep * img), no term added) ->
    (fp32 [N, HW, 4] with lane 3 = +0, fma_sums)"""
    if noise is None:
        v, sums = rn(f32(keep) * img.double()).float(), {}
    else:
        forms, sums = candidates_axpy(keep, mix, img, noise)
        v, sums = forms["A"], {"A": sums["A"]}
    out = torch.zeros(v.shape[0], v.shape[2], 4)
    out[..., :3] = nchw_as_pixels(v)
    return out, sums


@functools.lru_cache(maxsize=None)
def ambiguity_cases():
    """every (name, thunk -> fma_sums) whose unambiguity the GPU tests rely on: one per seeded input they form candidates from"""
    cases = []
    for n, hw in SHAPES:
        cases.append((f"img_prep {n}x{hw}", lambda n=n, hw=hw: expected_img_prep(KEEP, MIX, *make_img_prep(n, hw))[1]))
        for prec in (PREC_F32, PREC_BF16):
            def axpy(n=n, hw=hw, prec=prec):
                x, nz = make_axpy(n, hw, prec)
                return candidates_axpy(KEEP, MIX, x[..., :3], nchw_as_pixels(nz))[1]

            def interp(n=n, hw=hw, prec=prec):
                a, b, al = make_interp(n, hw, prec)
                return candidates_interp(al.view(n, 1, 1), a, b)[1]

            def tanh_bwd(n=n, hw=hw, prec=prec):
                return candidates_tanh_bwd(KEEP, *make_tanh_bwd(n, hw, prec))[1]
            cases += [(f"axpy {n}x{hw} prec {prec}", axpy), (f"interp {n}x{hw} prec {prec}", interp),
                      (f"tanh_bwd {n}x{hw} prec {prec}", tanh_bwd)]
    for prec in (PREC_F32, PREC_BF16):
        cases.append((f"tanh_bwd special prec {prec}", lambda prec=prec: candidates_tanh_bwd(KEEP, *make_tanh_special(prec))[1]))
    for hs, ws in U8_SHAPES:
        for idx in (U8_IDX, None):
            def u8(hs=hs, ws=ws, idx=idx):
                data, noise = make_u8(hs, ws)
                t = up2_pil_ref(data if idx is not None else data[:4], idx)
                return expected_img_prep(KEEP, MIX, t.flatten(2), noise.flatten(2))[1]
            cases.append((f"u8 {hs}x{ws} idx {idx}", u8))
    return tuple(cases)
