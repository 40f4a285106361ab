"""tests/image_ew_ref.py against exact rational arithmetic, the committed Pillow goldens and a numpy transcription of gp_norm_kernel's
summation order - the GPU tests of the image-side elementwise kernels (tests/test_image_ew_gpu.py) stand on this module.  No GPU."""
import hashlib
import json
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import image_ew_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


# ---- exact rational arithmetic ----------------------------------------------------------------------------------------------------
def _rn_frac(q):
    """the fp32 value nearest to the rational q, ties to even (normal range; the inputs below stay in it) -> Fraction"""
    if q == 0:
        return Fraction(0)
    s, a = (1, q) if q > 0 else (-1, -q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                      # 2^e <= a < 2^(e+1)
    assert -126 <= e <= 127
    ulp = Fraction(2) ** (e - 23)
    n, rem = divmod(a, ulp)
    if rem * 2 > ulp or (rem * 2 == ulp and n % 2):
        n += 1
    return s * n * ulp


def _fr(x):
    return Fraction(float(x))


def _inputs(count, seed, scale=1.0):
    """fp32 normals, some with few significant bits (bf16-like: exact products and sums, hence exact ties)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(count, generator=g) * scale
    x[::3] = x[::3].to(torch.bfloat16).float()
    return x


def _assert_forms(forms, want):
    """want: name -> list of Fractions"""
    for name, vals in want.items():
        got = forms[name].double().tolist()
        bad = [(i, g, float(v)) for i, (g, v) in enumerate(zip(got, vals)) if Fraction(g) != v]
        assert not bad, (name, len(bad), bad[:3])


def _tie_inputs():
    """(mix, nz, kx) with mix * nz + kx exactly half an fp32 ulp above / below an fp32 value, and one fp64 ulp to either side of such a
    midpoint: p = 1 + 2^-23 + d (d = 0, +-2^-24 ...) built as a product plus an addend"""
    rows = []
    for base in (1.0, 1.0 + 2.0 ** -23, 1.5, 1.0 + 3 * 2.0 ** -23):
        for nzv in (2.0 ** -24, -(2.0 ** -24), 2.0 ** -24 + 2.0 ** -47, 2.0 ** -24 - 2.0 ** -48, -(2.0 ** -24) - 2.0 ** -47,
                    3 * 2.0 ** -25, 2.0 ** -25):
            rows.append((1.0, nzv, base))            # 1 * nz + base: base + a half ulp, and a hair to either side
    return rows


def test_fma_candidates_against_fractions():
    """every candidate of axpy, interp and tanh_bwd on 300 random fp32 inputs (a third with few bits) and on values on both sides of
    fp32 ties, against Fractions rounded once per fp32 operation; where the fp64 route is ambiguous, fma_is_unambiguous says so"""
    keep, mix = R.f32(R.KEEP), R.f32(R.MIX)
    x, nz = _inputs(300, 1), _inputs(300, 2)
    forms, sums = R.candidates_axpy(R.KEEP, R.MIX, x, nz)
    assert R.ambiguous_count(sums) == 0
    K, M = Fraction(keep), Fraction(mix)
    _assert_forms(forms, {
        "A": [_rn_frac(M * _fr(b) + _rn_frac(K * _fr(a))) for a, b in zip(x, nz)],
        "B": [_rn_frac(_rn_frac(K * _fr(a)) + _rn_frac(M * _fr(b))) for a, b in zip(x, nz)],
        "C": [_rn_frac(K * _fr(a) + _rn_frac(M * _fr(b))) for a, b in zip(x, nz)]})
    assert not torch.equal(forms["A"], forms["B"]) and not torch.equal(forms["A"], forms["C"]) and not torch.equal(forms["B"], forms["C"])

    a, b, al = _inputs(300, 3), _inputs(300, 4), torch.rand(300, generator=torch.Generator().manual_seed(5))
    forms, sums = R.candidates_interp(al, a, b)
    assert R.ambiguous_count(sums) == 0
    t = [_rn_frac(1 - _fr(v)) for v in al]
    _assert_forms(forms, {
        "U": [_rn_frac(_rn_frac(_fr(l) * _fr(p)) + _rn_frac(tt * _fr(q))) for l, tt, p, q in zip(al, t, a, b)],
        "Fa": [_rn_frac(_fr(l) * _fr(p) + _rn_frac(tt * _fr(q))) for l, tt, p, q in zip(al, t, a, b)],
        "Fb": [_rn_frac(tt * _fr(q) + _rn_frac(_fr(l) * _fr(p))) for l, tt, p, q in zip(al, t, a, b)]})
    assert len({tuple(R.bits(f).tolist()) for f in forms.values()}) == 3

    g, y = _inputs(300, 6), torch.tanh(_inputs(300, 7, 1.5))
    y[:4] = torch.tensor([1.0, -1.0, 0.0, 1.0 - 2.0 ** -24])
    forms, sums = R.candidates_tanh_bwd(R.KEEP, g, y)
    assert R.ambiguous_count(sums) == 0
    q = [_rn_frac(K * _fr(v)) for v in g]
    _assert_forms(forms, {
        "U": [_rn_frac(qq * _rn_frac(1 - _rn_frac(_fr(v) * _fr(v)))) for qq, v in zip(q, y)],
        "F": [_rn_frac(qq * _rn_frac(1 - _fr(v) * _fr(v))) for qq, v in zip(q, y)]})
    assert not torch.equal(forms["U"], forms["F"])
    # y = 1 - 2^-24: 1 - y^2 = 2^-23 - 2^-48 is an exact tie between 2^-23 - 2^-47 and 2^-23 and goes to the even 2^-23, which is
    # what 1 - rn(y^2) gives too: the two forms agree at this y (and the fp64 sum, being exact, is not ambiguous)
    assert forms["U"][3] == forms["F"][3] == float(np.float32(keep * float(g[3])) * np.float32(2.0 ** -23))
    assert forms["U"][0] == 0 and forms["U"][1] == 0 and forms["F"][0] == 0 and forms["F"][1] == 0
    assert forms["U"][2] == forms["F"][2] == float(np.float32(keep * float(g[2])))


def test_fma_at_ties():
    """mix * nz + kx on, and one hair to either side of, the midpoint of two fp32 values: the exact sums (ties and near-ties that fp64
    holds exactly) round as the Fractions do and count as unambiguous through the exactness mask; without the mask every one of them
    within 2^-50 of the midpoint is flagged"""
    rows = _tie_inputs()
    one, nz, kx = (torch.tensor([r[i] for r in rows], dtype=torch.float64) for i in range(3))
    assert torch.equal(nz.float().double(), nz) and torch.equal(kx.float().double(), kx)
    s, exact = R._fma(one, nz, kx)
    assert bool(exact.all())
    want = [_rn_frac(Fraction(r[1]) + Fraction(r[2])) for r in rows]
    assert [Fraction(v) for v in s.float().double().tolist()] == want
    assert bool(R.fma_is_unambiguous(s, exact).all())
    flagged = ~R.fma_is_unambiguous(s)
    mid_dist = torch.tensor([abs(Fraction(r[1]) + Fraction(r[2]) - _mid(Fraction(r[1]) + Fraction(r[2]))) / (Fraction(r[1]) + Fraction(r[2]))
                             for r in rows], dtype=torch.float64)
    assert torch.equal(flagged, mid_dist <= 2.0 ** -50), (flagged.tolist(), mid_dist.tolist())
    assert int(flagged.sum()) >= 4 and int((~flagged).sum()) >= 8


def _mid(q):
    """the midpoint nearest to q > 0 of two neighbouring fp32 values"""
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    return (q // ulp) * ulp + ulp / 2


def test_an_inexact_sum_beside_a_midpoint_is_ambiguous():
    """a = 32 + 2^-18, b = 1 - 2^-23 (fp32 values): a * b = 32 - 2^-41.  Added to c = 2^29 (fp32 spacing 64, fp64 spacing 2^-23) the
    exact sum lies 2^-41 below the midpoint c + 32, fp64 lands ON the midpoint, and the second rounding goes to the even neighbour:
    right for c = 2^29, wrong for c = 2^29 + 64.  fma_is_unambiguous flags both; a sum 2^-46 relative from the midpoint passes."""
    a = torch.tensor([32.0 + 2.0 ** -18], dtype=torch.float64)
    b = torch.tensor([1.0 - 2.0 ** -23], dtype=torch.float64)
    assert torch.equal(a.float().double(), a) and torch.equal(b.float().double(), b)
    for c0, via_fp64, fma in ((2.0 ** 29, 2.0 ** 29, 2.0 ** 29), (2.0 ** 29 + 64.0, 2.0 ** 29 + 128.0, 2.0 ** 29 + 64.0)):
        c = torch.tensor([c0], dtype=torch.float64)
        s, exact = R._fma(a, b, c)
        assert not bool(exact[0]) and s.item() == c0 + 32.0
        assert not bool(R.fma_is_unambiguous(s, exact)[0]) and not bool(R.fma_is_unambiguous(s)[0])
        assert s.float().item() == via_fp64
        assert _rn_frac(Fraction(a.item()) * Fraction(b.item()) + Fraction(c0)) == Fraction(fma)
    b = torch.tensor([1.0 + 2.0 ** -23], dtype=torch.float64)                    # a * b = 32 + 2^-17 + 2^-41
    s, exact = R._fma(a, b, torch.tensor([2.0 ** 29], dtype=torch.float64))
    assert not bool(exact[0]) and bool(R.fma_is_unambiguous(s, exact)[0]) and s.float().item() == 2.0 ** 29 + 64.0
    assert bool(R.fma_is_unambiguous(torch.tensor([math.inf, math.nan, 0.0, 1.0, 3e38, 1e-45, 1e300], dtype=torch.float64)).all())


def test_gp_grad_reference_against_fractions():
    g = torch.Generator().manual_seed(8)
    v = torch.randn(200, generator=g) * 0.02
    nr = torch.rand(200, generator=g) * 2 + 0.25
    nr[:3] = torch.tensor([0.0, 1.0, math.nan])
    coef = R.f32(2 * 10.0 / 5)
    got = R.candidates_gp_grad(coef, nr, v)[0]["one"].double().tolist()
    for i in range(200):
        n = float(nr[i])
        f = _rn_frac(_rn_frac(Fraction(coef) * _rn_frac(Fraction(n) - 1)) / Fraction(n)) if n > 0 else Fraction(0)
        assert Fraction(got[i]) == _rn_frac(_fr(v[i]) * f), i
    assert got[0] == 0 and got[1] == 0 and got[2] == 0                            # norm 0, norm 1, NaN norm (f = 0)


# ---- Pillow -----------------------------------------------------------------------------------------------------------------------
def test_up2_pil_ref_reproduces_the_pillow_goldens():
    """tests/golden/resize_u8.json as test_preprocess_cpu.py checks it (digest, sum, the full small case, the samples), and the fp32
    transform against the oracle's, which test_preprocess_gpu.py holds jck_img_prep_u8 to"""
    from make_golden_resize import inputs
    from oracle.preprocess_oracle import transform
    gold = json.load(open(os.path.join(HERE, "golden", "resize_u8.json")))
    for case in gold["cases"].values():
        x = inputs(case["seed"], case["n"], case["h"])
        y = R.up2_pil_u8(torch.from_numpy(x)).numpy()
        assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == case["sha256"]
        assert int(y.astype(np.int64).sum()) == case["sum"]
        if "full" in case:
            assert np.array_equal(y, np.asarray(case["full"], dtype=np.uint8))
        for n, c, yy, xx, v in case.get("samples", []):
            assert int(y[n, c, yy, xx]) == v
    x = inputs(7, 6, 32)
    idx = [5, 0, 3, 3, 1]
    assert np.array_equal(R.up2_pil_ref(torch.from_numpy(x), idx).numpy(), transform(x)[idx])


def test_up2_pil_ref_at_one_pixel_sources():
    """a one-pixel-wide or -high source: both clamped taps are the pixel itself, (3a + a + 2) >> 2 = a; Hs != Ws keeps its axes"""
    for hs, ws in R.U8_SHAPES:
        data, _ = R.make_u8(hs, ws)
        y = R.up2_pil_u8(data)
        assert y.shape == (5, 3, 2 * hs, 2 * ws)
        if ws == 1:
            assert torch.equal(y[..., 0], y[..., 1])
        if hs == 1:
            assert torch.equal(y[..., 0, :], y[..., 1, :])
        if hs == 1 and ws == 1:
            assert torch.equal(y, data.expand(5, 3, 2, 2))
        # the plain loop, one output pixel at a time
        a = data.to(torch.int64)
        for (n, c, oy, ox) in [(2, 1, 0, 0), (3, 2, 2 * hs - 1, 2 * ws - 1), (4, 0, hs, ws), (1, 0, 2 * hs - 1, 0)]:
            def hpass(r):
                k = ox >> 1
                m, p = max(k - 1, 0), min(k + 1, ws - 1)
                return (3 * a[n, c, r, k] + a[n, c, r, p] + 2) >> 2 if ox & 1 else (a[n, c, r, m] + 3 * a[n, c, r, k] + 2) >> 2
            k = oy >> 1
            m, p = max(k - 1, 0), min(k + 1, hs - 1)
            want = (3 * hpass(k) + hpass(p) + 2) >> 2 if oy & 1 else (hpass(m) + 3 * hpass(k) + 2) >> 2
            assert int(y[n, c, oy, ox]) == int(want), (hs, ws, n, c, oy, ox)


# ---- the inputs of the GPU tests are unambiguous ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(R.ambiguity_cases())), ids=[c[0].replace(" ", "-") for c in R.ambiguity_cases()])
def test_gpu_inputs_are_unambiguous(case):
    """every seed and shape of tests/test_image_ew_gpu.py: the number of elements at which an fma candidate's fp64 route could round
    the other way is exactly 0"""
    name, thunk = R.ambiguity_cases()[case]
    assert R.ambiguous_count(thunk()) == 0, name


# ---- gp_norm ----------------------------------------------------------------------------------------------------------------------
def test_gp_norm_bound():
    assert R.gp_norm_bound(1) == R.gp_norm_bound(256) == (14 / 2 + 1) * 2.0 ** -24
    assert R.gp_norm_bound(257) == (19 / 2 + 1) * 2.0 ** -24
    assert R.gp_norm_bound(16384) == ((5 * 64 + 9) / 2 + 1) * 2.0 ** -24
    for p in (1, 255, 257, 4096):
        for prec in (R.PREC_F32, R.PREC_BF16):
            g = R.make_gp_norm(3, p, prec)
            for n in range(3):
                ref = float(g[n].double().pow(2).sum().sqrt())
                got = float(R.gp_norm_sim(g[n].numpy()))
                if n == 1:
                    assert got == 0.0 and ref == 0.0
                    continue
                err = abs(got - ref) / ref
                print(f"gp_norm_sim P={p} prec={prec} image {n}: rel err {err:.3e}, bound {R.gp_norm_bound(p):.3e}")
                assert err <= R.gp_norm_bound(p), (p, prec, n, err)
    # the simulation is the kernel's order and not any order: a thread's groups are 256 apart
    g = np.zeros((512, 4), np.float32)
    g[0, 0], g[256, 0], g[1, 0] = 1.0, 2.0 ** -13, 2.0 ** -13                    # squares 1, 2^-26, 2^-26
    assert R.gp_norm_sim(g) == np.sqrt(np.float32(1.0) + np.float32(2.0 ** -26))  # (1 + 2^-26) = 1 in the thread, then + 2^-26 = 1 again


def test_seeds_are_distinct():
    seeds = [R.seed_of(k, c, p) for k in ("axpy", "interp", "tanh_bwd", "gp_grad") for c in R.SHAPES for p in (0, 1)]
    seeds += [R.seed_of("gp_norm", c, p) for c in R.GP_NORM_CASES for p in (0, 1)] + [R.seed_of("u8", c, 1) for c in R.U8_SHAPES]
    assert len(set(seeds)) == len(seeds)
