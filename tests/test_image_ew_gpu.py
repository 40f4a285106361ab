"""The image-side elementwise kernels of csrc/ew.hpp through the C ABI, bit for bit against tests/image_ew_ref.py (pinned on the CPU by
tests/test_image_ew_ref_cpu.py): jck_img_prep, jck_axpy_noise, jck_mix_interp, jck_interp, jck_nhwc4_to_nchw, jck_tanh_bwd, jck_gp_norm,
jck_gp_grad, jck_img_prep_u8 - at one pixel, at an odd HW (image boundaries inside a wave), at today's 3 x 4096, and past ew_grid's cap
of 8192 x 256 items (the grid-stride loop takes a second trip), in fp32 and bf16 storage; every output sits in a buffer 64 elements
longer than it needs, with a sentinel behind the end that must stay.

What is asserted bit for bit: the expected value is formed in fp64 from the values the kernel reads and rounded once per fp32 operation
(image_ew_ref), then, for bf16 storage, to bf16 with round-to-nearest-even.  Where the compiler may or may not contract a multiply-add,
every legal contraction is a candidate; a launch must equal ONE candidate in all its elements (both grid trips), and the candidate is
the one recorded in FORMS below - a compiler update or a refactor that moves the step's bits fails here first.  The tests assert of
their INPUTS that no fma candidate lies where fp64-then-fp32 rounding could differ from the fma (image_ew_ref.fma_is_unambiguous).

Contraction forms found on the MI355X (hipcc -O3, its default -ffp-contract=fast-honor-pragmas), the same in fp32 and bf16 storage:
  img_prep, img_prep_u8   A   fma(mix, nz, rn(keep * x))             pinned by __fmaf_rn (__fmul_rn and __fadd_rn are the plain
                                                                     operators in this toolchain and would be contracted again)
  axpy_noise              A   fma(mix, nz, rn(keep * x))             v_mul_f32, v_fma_f32: the promise in img_prep_kernel's comment holds
  interp (and mix_interp) Fa  fma(al, a, rn(rn(1 - al) * b))         v_pk_mul_f32, v_pk_fma_f32
  tanh_bwd                F   rn(rn(scale * g) * fma(-y, y, 1))      v_pk_fma_f32 with a negated operand
  gp_grad                 one rn(v * rn(rn(coef * rn(nr - 1)) / nr)) nothing to contract
At y = 1 - 2^-24 both tanh_bwd forms give rn(scale * g) * 2^-23: the fused 1 - y^2 = 2^-23 - 2^-48 is an exact tie and goes to the even
2^-23, which is what 1 - rn(y^2) gives; the forms differ most (2^-13 relative) near y = 1 - 2^-12, and at random y in a share of elements.
In bf16 storage y * y has 16 bits and is exact in fp32, so tanh_bwd's two forms are one and the same there; at (1, 1), and in bf16 storage
at (5, 37), the candidates of the other kernels coincide too - the larger shapes tell them apart.

gp_norm: max |norm - fp64 norm| / fp64 norm measured on the MI355X beside image_ew_ref.gp_norm_bound (derived, not tuned), fp32 | bf16
storage, over the images of the case:
  per_image4      1: 4.61e-08 | 3.37e-08   bound 4.77e-07
  per_image4    255: 2.12e-08 | 2.29e-08   bound 4.77e-07
  per_image4    256: 5.58e-08 | 4.57e-08   bound 4.77e-07
  per_image4    257: 1.02e-08 | 1.47e-08   bound 6.26e-07
  per_image4   4096: 1.31e-08 | 6.15e-08   bound 2.71e-06
  per_image4  16384: 4.46e-08 | 2.66e-08   bound 9.87e-06
  per_image4     64: 8.68e-08 | 8.91e-08   bound 4.77e-07   (N = 300)
The errors do not grow with per_image4 as the bound does: the bound counts every rounding as if all went one way.

Non-finite values in jck_gp_grad, as the kernel behaves today (recorded, not a statement of what it should do): a NaN or infinite
element of g gives a non-finite element of u and leaves the image's other elements alone, because the norm is an input of the kernel;
a NaN norm fails `nr > 0` and gives f = 0: u = +-0 at every finite element of that image (NaN at a non-finite one); an infinite norm
gives f = inf / inf = NaN: u = NaN in the whole image.  torch autograd of coef / 2 * sum_n (||g_n|| - 1)^2, which forms the norm from g
itself, gives NaN in EVERY element of an image that holds a NaN or an infinite element, and 0 nowhere.

None of these kernels has a launch name (the registry gives img_prep_u8 a profiler label only): jck_last_launch must say after every
test of this module what it said before."""
import math

import pytest
import torch

import image_ew_ref as R

pytestmark = pytest.mark.gpu

PRECS = [1, 0]
SENT = -3.25                                        # behind the end of every output; exact in bf16
GUARD = 64
KEEP, MIX = R.KEEP, R.MIX
FORMS = {"axpy": {1: "A", 0: "A"}, "interp": {1: "Fa", 0: "Fa"}, "tanh_bwd": {1: "F", 0: "F"}, "gp_grad": {1: "one", 0: "one"}}


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


@pytest.fixture(autouse=True)
def _no_launch_name(G):
    before = G.lib.jck_last_launch()
    yield
    assert G.lib.jck_last_launch() == before


def _ids(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else None


def _dev(x, prec):
    return x.to(R.DT[prec]).cuda().contiguous()


def _out(numel, dt, fill=math.nan):
    """a flat device buffer of numel + GUARD elements: `fill` where the kernel must write, SENT behind the end"""
    t = torch.full((numel + GUARD,), fill, dtype=dt, device="cuda")
    t[numel:] = SENT
    return t


def _take(buf, numel, what):
    """-> the first numel elements on the CPU; the sentinel behind them must have stayed"""
    torch.cuda.synchronize()
    t = buf.cpu()
    assert bool((t[numel:].float() == SENT).all()), f"{what}: wrote behind the end"
    return t[:numel]


def _same(got, want32, prec):
    """got (stored type) equals the fp32 expectation as stored, bit for bit"""
    return torch.equal(R.bits(got), R.bits(R.store(want32, prec).reshape(got.shape)))


def _assert_same(got, want32, prec, what):
    g, w = R.bits(got), R.bits(R.store(want32, prec).reshape(got.shape))
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w).flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {g.numel()} elements differ, first at {i}: got {got.flatten()[i].item().hex()} "
                             f"want {R.store(want32, prec).flatten()[i].item().hex()}")


def _one_form(got, forms, prec, kernel, what):
    """all elements of the launch equal the same candidate, and it is the recorded one"""
    hits = [k for k, v in forms.items() if _same(got, v, prec)]
    print(f"{what}: equals candidate(s) {hits} of {list(forms)}; recorded {FORMS[kernel][prec]}")
    if FORMS[kernel][prec] not in hits:
        _assert_same(got, forms[FORMS[kernel][prec]], prec, f"{what} (candidates equal in every element: {hits})")


def _lane3_zero(got4, what):
    assert bool((R.bits(got4[..., 3].contiguous()) == 0).all()), f"{what}: lane 3 is not +0"


def _raises_and_leaves(G, call, bufs, what):
    """the call raises JckError and every buffer keeps its bits"""
    from hipgan._lib import JckError
    before = [b.clone() for b in bufs]
    with pytest.raises(JckError):
        call()
    torch.cuda.synchronize()
    for b, c in zip(bufs, before):
        assert torch.equal(R.bits(b), R.bits(c)), f"{what}: a refused call wrote"


# ---- img_prep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_img_prep(G, shape, prec):
    """out = rn_T(fma(mix, noise, rn(keep * img))) in lanes 0..2, +0 in lane 3; noise = NULL adds no term; keep, mix = 1, 0 gives
    rn_T(img) with and without a noise tensor (fma(0, nz, img) = img)"""
    n, hw = shape
    img, nz = R.make_img_prep(n, hw)
    want, sums = R.expected_img_prep(KEEP, MIX, img, nz)
    assert R.ambiguous_count(sums) == 0
    plain = torch.zeros(n, hw, 4)
    plain[..., :3] = R.nchw_as_pixels(img)
    cases = [("0.9/0.1", KEEP, MIX, nz, want), ("1/0 with noise", 1.0, 0.0, nz, plain), ("1/0", 1.0, 0.0, None, plain),
             ("0.9/0.1 no noise", KEEP, MIX, None, R.expected_img_prep(KEEP, MIX, img, None)[0])]
    dimg, dnz = img.cuda(), nz.cuda()
    for name, keep, mix, noise, exp in cases:
        out = _out(n * hw * 4, R.DT[prec])
        G.lib.jck_img_prep(prec, dimg, None if noise is None else dnz, keep, mix, out, n, hw, G.cur_stream())
        got = _take(out, n * hw * 4, f"img_prep {name}").view(n, hw, 4)
        _assert_same(got, exp, prec, f"img_prep {name} {shape} prec {prec}")
        _lane3_zero(got, f"img_prep {name}")


# ---- axpy_noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_axpy_noise(G, shape, prec):
    """one candidate of keep * x + mix * nz in every element; lane 3 of x holds NaN and lane 3 of the output is +0"""
    n, hw = shape
    x, nz = R.make_axpy(n, hw, prec)
    forms, sums = R.candidates_axpy(KEEP, MIX, x[..., :3], R.nchw_as_pixels(nz))
    assert R.ambiguous_count(sums) == 0
    out = _out(n * hw * 4, R.DT[prec])
    G.lib.jck_axpy_noise(prec, _dev(x, prec), nz.cuda(), KEEP, MIX, out, n, hw, G.cur_stream())
    got = _take(out, n * hw * 4, "axpy_noise").view(n, hw, 4)
    _lane3_zero(got, "axpy_noise")
    _one_form(got[..., :3].contiguous(), forms, prec, "axpy", f"axpy_noise {shape} prec {prec}")
    # noise = NULL (and no rng): keep * x alone
    out = _out(n * hw * 4, R.DT[prec])
    G.lib.jck_axpy_noise(prec, _dev(x, prec), None, KEEP, MIX, out, n, hw, G.cur_stream())
    got = _take(out, n * hw * 4, "axpy_noise, no noise").view(n, hw, 4)
    _lane3_zero(got, "axpy_noise, no noise")
    _assert_same(got[..., :3].contiguous(), R.rn(R.f32(KEEP) * x[..., :3].double()).float(), prec, "axpy_noise, no noise")


@pytest.mark.parametrize("shape", [(5, 37), (3, 700_001)], ids=_ids)
def test_axpy_noise_rounds_as_img_prep(G, shape):
    """the promise in img_prep_kernel's comment, "the same rounding in every kernel that mixes noise": with x the fp32 image,
    jck_axpy_noise(x, nz) is jck_img_prep(img, nz) bit for bit in fp32 storage - true only while axpy_noise compiles to form A"""
    n, hw = shape
    img, nz = R.make_img_prep(n, hw)
    x = torch.full((n, hw, 4), math.nan)
    x[..., :3] = R.nchw_as_pixels(img)
    a, b = _out(n * hw * 4, torch.float32), _out(n * hw * 4, torch.float32)
    G.lib.jck_img_prep(1, img.cuda(), nz.cuda(), KEEP, MIX, a, n, hw, G.cur_stream())
    G.lib.jck_axpy_noise(1, x.cuda(), nz.cuda(), KEEP, MIX, b, n, hw, G.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(R.bits(a), R.bits(b))
    assert FORMS["axpy"][1] == "A"


# ---- interp -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_interp(G, shape, prec):
    """one candidate of al[n] * a + (1 - al[n]) * b in every element of all four lanes; the pixels on both sides of every image
    boundary take their own image's alpha (and would differ with the neighbour's)"""
    n, hw = shape
    a, b, al = R.make_interp(n, hw, prec)
    forms, sums = R.candidates_interp(al.view(n, 1, 1), a, b)
    assert R.ambiguous_count(sums) == 0
    out = _out(n * hw * 4, R.DT[prec])
    G.lib.jck_interp(prec, _dev(a, prec), _dev(b, prec), al.cuda(), out, n, hw, G.cur_stream())
    got = _take(out, n * hw * 4, "interp").view(n, hw, 4)
    _one_form(got, forms, prec, "interp", f"interp {shape} prec {prec}")
    form = FORMS["interp"][prec]
    for k in range(n - 1):                          # last pixel of image k, first pixel of image k + 1
        for img, px, other in ((k, hw - 1, k + 1), (k + 1, 0, k)):
            own = R.candidates_interp(al[img], a[img, px], b[img, px])[0][form]
            wrong = R.candidates_interp(al[other], a[img, px], b[img, px])[0][form]
            assert not _same(R.store(own, prec), wrong, prec), "the boundary pixel cannot tell the two alphas apart: change the seed"
            _assert_same(got[img, px], own, prec, f"interp image {img} pixel {px}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(5, 37), (3, 4096)], ids=_ids)
def test_interp_alpha_one_and_zero(G, shape, prec):
    """alpha exactly 1 gives a, alpha exactly 0 gives b, bit for bit (images take turns, so both happen in one launch)"""
    n, hw = shape
    a, b, _ = R.make_interp(n, hw, prec)
    al = torch.tensor([float(i % 2) for i in range(n)])
    out = _out(n * hw * 4, R.DT[prec])
    G.lib.jck_interp(prec, _dev(a, prec), _dev(b, prec), al.cuda(), out, n, hw, G.cur_stream())
    got = _take(out, n * hw * 4, "interp").view(n, hw, 4)
    for i in range(n):
        _assert_same(got[i], (a if i % 2 else b)[i], prec, f"interp alpha {i % 2}")


# ---- mix_interp -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(5, 37), (3, 700_001)], ids=_ids)
def test_mix_interp_is_the_two_launches(G, shape, prec):
    """explicit noise: `out` and `xhat` of the one launch are jck_axpy_noise's and jck_interp(real, out, alpha)'s bits"""
    n, hw = shape
    x, nz = R.make_axpy(n, hw, prec)
    real, _, al = R.make_interp(n, hw, prec)
    dx, dnz, dreal, dal = _dev(x, prec), nz.cuda(), _dev(real, prec), al.cuda()
    num = n * hw * 4
    o1, h1, o2, h2 = (_out(num, R.DT[prec]) for _ in range(4))
    G.lib.jck_axpy_noise(prec, dx, dnz, KEEP, MIX, o1, n, hw, G.cur_stream())
    G.lib.jck_interp(prec, dreal, o1, dal, h1, n, hw, G.cur_stream())
    G.lib.jck_mix_interp(prec, dx, dnz, None, 0, KEEP, MIX, o2, dreal, dal, h2, n, hw, G.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(R.bits(o1), R.bits(o2)), "mix_interp: out"
    assert torch.equal(R.bits(h1), R.bits(h2)), "mix_interp: xhat"
    assert not bool(torch.isnan(h1[:num].float()).any())


def test_mix_interp_refusals(G):
    """real, alpha or xhat NULL, and noise and rng both given or both missing: JckError, nothing written"""
    n, hw, prec = 5, 37, 1
    x, nz = R.make_axpy(n, hw, prec)
    real, _, al = R.make_interp(n, hw, prec)
    dx, dnz, dreal, dal = x.cuda(), nz.cuda(), real.cuda(), al.cuda()
    rng = torch.tensor([1, 2, 3, 0], dtype=torch.int32, device="cuda")
    out, xhat = _out(n * hw * 4, torch.float32, 5.0), _out(n * hw * 4, torch.float32, 6.0)
    st = G.cur_stream()
    for what, args in (("real", (dnz, None, out, None, dal, xhat)), ("alpha", (dnz, None, out, dreal, None, xhat)),
                       ("xhat", (dnz, None, out, dreal, dal, None)), ("noise and rng", (dnz, rng, out, dreal, dal, xhat)),
                       ("neither noise nor rng", (None, None, out, dreal, dal, xhat))):
        noise, r, o, re, a, xh = args
        _raises_and_leaves(G, lambda: G.lib.jck_mix_interp(prec, dx, noise, r, 0, KEEP, MIX, o, re, a, xh, n, hw, st), [out, xhat],
                           f"mix_interp without {what}")


# ---- nhwc4_to_nchw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_nhwc4_to_nchw(G, shape, prec):
    """an exact permutation of lanes 0..2 (widened to fp32); lane 3 holds NaN and leaves no trace"""
    n, hw = shape
    x, _ = R.make_axpy(n, hw, prec)
    out = _out(n * 3 * hw, torch.float32)
    G.lib.jck_nhwc4_to_nchw(prec, _dev(x, prec), out, n, hw, G.cur_stream())
    got = _take(out, n * 3 * hw, "nhwc4_to_nchw").view(n, 3, hw)
    assert torch.equal(R.bits(got), R.bits(x[..., :3].permute(0, 2, 1).contiguous()))
    assert not bool(torch.isnan(got).any())


# ---- tanh_bwd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_tanh_bwd(G, shape, prec):
    """one candidate of scale * g * (1 - y * y) in every element"""
    n, hw = shape
    g, y = R.make_tanh_bwd(n, hw, prec)
    forms, sums = R.candidates_tanh_bwd(KEEP, g, y)
    assert R.ambiguous_count(sums) == 0
    out = _out(n * hw * 4, R.DT[prec])
    G.lib.jck_tanh_bwd(prec, _dev(g, prec), _dev(y, prec), KEEP, out, n * hw * 4, G.cur_stream())
    got = _take(out, n * hw * 4, "tanh_bwd").view(n, hw, 4)
    _one_form(got, forms, prec, "tanh_bwd", f"tanh_bwd {shape} prec {prec}")


@pytest.mark.parametrize("prec", PRECS)
def test_tanh_bwd_special_values(G, prec):
    """y = +-1 gives exactly 0, y = 0 gives rn(scale * g); in fp32, y = 1 - 2^-24 (both forms: rn(scale * g) * 2^-23, see the module
    docstring) and y = 1 - 2^-12 + k 2^-24 around where the forms differ most each equal the recorded candidate bit for bit"""
    g, y = R.make_tanh_special(prec)
    forms, sums = R.candidates_tanh_bwd(KEEP, g, y)
    assert R.ambiguous_count(sums) == 0
    if prec == 1:
        assert not torch.equal(R.bits(forms["U"]), R.bits(forms["F"])) and forms["U"][4] == forms["F"][4]
    out = _out(64, R.DT[prec])
    G.lib.jck_tanh_bwd(prec, _dev(g, prec), _dev(y, prec), KEEP, out, 64, G.cur_stream())
    got = _take(out, 64, "tanh_bwd")
    _one_form(got, forms, prec, "tanh_bwd", f"tanh_bwd special values prec {prec}")
    assert bool((got[:2].float() == 0).all())
    _assert_same(got[2:4], R.rn(R.f32(KEEP) * g[2:4].double()).float(), prec, "tanh_bwd at y = 0")


@pytest.mark.parametrize("prec", PRECS)
def test_tanh_bwd_refuses_a_ragged_count(G, prec):
    g = torch.ones(8, dtype=R.DT[prec], device="cuda")
    out = _out(8, R.DT[prec], 5.0)
    for numel in (1, 2, 3, 7):
        _raises_and_leaves(G, lambda: G.lib.jck_tanh_bwd(prec, g, g, KEEP, out, numel, G.cur_stream()), [out], f"tanh_bwd numel {numel}")


# ---- gp_norm ----------------------------------------------------------------------------------------------------------------------
def _gp_norm(G, prec, g, n, p, scal, slot, ld, norms):
    G.lib.jck_gp_norm(prec, g, n, p, scal, slot, ld, norms, G.cur_stream())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.GP_NORM_CASES, ids=_ids)
def test_gp_norm(G, case, prec):
    """norms within gp_norm_bound of fp64; the penalty slot bit for bit rn(rn(nr - 1) * rn(nr - 1)) of the kernel's own norms; the zero
    image gives norm 0 and penalty 1 exactly; the rest of a NaN-filled table stays NaN; two launches give equal bits"""
    n, p = case
    v = R.make_gp_norm(n, p, prec)
    g = _dev(v, prec)
    slots, ld, slot = 8, n + 3, 6
    scal = _out(slots * ld, torch.float32)
    norms = _out(n, torch.float32)
    _gp_norm(G, prec, g, n, p, scal, slot, ld, norms)
    nr = _take(norms, n, "gp_norm norms")
    table = _take(scal, slots * ld, "gp_norm table").view(slots, ld)
    ref = v.double().reshape(n, -1).pow(2).sum(1).sqrt()
    assert nr[1].item() == 0.0 and R.bits(nr[1:2]).item() == 0 and table[slot, 1].item() == 1.0
    live = ref > 0
    err = ((nr.double() - ref).abs()[live] / ref[live]).max().item()
    print(f"gp_norm N={n} per_image4={p} prec={prec}: max rel err {err:.3e}, bound {R.gp_norm_bound(p):.3e}")
    assert err <= R.gp_norm_bound(p)
    assert torch.equal(R.bits(table[slot, :n].contiguous()), R.bits((nr - 1.0) * (nr - 1.0)))
    mask = torch.ones(slots, ld, dtype=torch.bool)
    mask[slot, :n] = False
    assert bool(torch.isnan(table[mask]).all()), "gp_norm wrote table entries it does not own"
    scal2, norms2 = _out(slots * ld, torch.float32), _out(n, torch.float32)
    _gp_norm(G, prec, g, n, p, scal2, slot, ld, norms2)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(norms), R.bits(norms2)) and torch.equal(R.bits(scal), R.bits(scal2))


@pytest.mark.parametrize("prec", PRECS)
def test_gp_norm_optional_outputs(G, prec):
    """slot = -1 and scal = NULL leave the table alone and still write the norms; norms = NULL still writes the penalties;
    scal_ld < N raises and writes nothing (and is not checked where no table is written)"""
    n, p, slots, ld = 3, 257, 8, 5
    g = _dev(R.make_gp_norm(n, p, prec), prec)
    scal, norms = _out(slots * ld, torch.float32), _out(n, torch.float32)
    _gp_norm(G, prec, g, n, p, scal, 2, ld, norms)
    want_nr, want_pen = _take(norms, n, "norms").clone(), _take(scal, slots * ld, "table").view(slots, ld)[2, :n].clone()
    for what, tab, slot, l in (("slot -1", True, -1, ld), ("no table", False, 2, ld), ("slot -1, short table", True, -1, 1),
                               ("no table, short ld", False, 2, 1)):
        scal, norms = _out(slots * ld, torch.float32), _out(n, torch.float32)
        _gp_norm(G, prec, g, n, p, scal if tab else None, slot, l, norms)
        assert torch.equal(R.bits(_take(norms, n, what)), R.bits(want_nr)), what
        assert bool(torch.isnan(_take(scal, slots * ld, what)).all()), what
    scal = _out(slots * ld, torch.float32)
    _gp_norm(G, prec, g, n, p, scal, 2, ld, None)
    table = _take(scal, slots * ld, "no norms").view(slots, ld)
    assert torch.equal(R.bits(table[2, :n].contiguous()), R.bits(want_pen))
    table[2, :n] = math.nan
    assert bool(torch.isnan(table).all())
    scal, norms = _out(slots * ld, torch.float32), _out(n, torch.float32)
    _raises_and_leaves(G, lambda: _gp_norm(G, prec, g, n, p, scal, 2, n - 1, norms), [scal, norms], "gp_norm scal_ld < N")


# ---- gp_grad ----------------------------------------------------------------------------------------------------------------------
COEF = 2 * 10.0 / 5


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_gp_grad(G, shape, prec):
    """u = rn_T(rn(v * f)), f = rn(rn(coef * rn(nr - 1)) / nr) of the image's own norm (0 for norm 0), in every element; the elements on
    both sides of every image boundary take their own image's norm (and would differ with the neighbour's)"""
    n, hw = shape
    v, nr = R.make_gp_grad(n, hw, prec)
    forms, _ = R.candidates_gp_grad(COEF, nr.view(n, 1, 1), v)
    out = _out(n * hw * 4, R.DT[prec])
    G.lib.jck_gp_grad(prec, _dev(v, prec), nr.cuda(), COEF, n, hw, out, G.cur_stream())
    got = _take(out, n * hw * 4, "gp_grad").view(n, hw, 4)
    _one_form(got, forms, prec, "gp_grad", f"gp_grad {shape} prec {prec}")
    if n == 5:
        assert bool((got[3].float() == 0).all()), "norm 0 must give u = 0"
    for k in range(n - 1):
        for img, px, other in ((k, hw - 1, k + 1), (k + 1, 0, k)):
            own = R.candidates_gp_grad(COEF, nr[img], v[img, px])[0]["one"]
            wrong = R.candidates_gp_grad(COEF, nr[other], v[img, px])[0]["one"]
            assert not _same(R.store(own, prec), wrong, prec), "the boundary pixel cannot tell the two norms apart: change the seed"
            _assert_same(got[img, px], own, prec, f"gp_grad image {img} pixel {px}")


@pytest.mark.parametrize("prec", PRECS)
def test_gp_grad_non_finite_as_today(G, prec):
    """Today's behaviour, recorded: a NaN or infinite element of g stays non-finite in u and the image's other elements keep their
    values; a NaN norm gives f = 0 (`nr > 0` is false): +-0 at finite elements, NaN at non-finite ones; an infinite norm gives
    f = NaN: the whole image NaN.  torch autograd of coef / 2 * sum (||g_n|| - 1)^2 on the same g gives NaN in every element of an
    image with a NaN or infinite element: the kernel is handed the norm and does not see the element."""
    n, hw = 4, 37
    v, _ = R.make_gp_grad(n, hw, prec)
    v = v[:n].clone()
    nr = torch.tensor([0.75, math.nan, math.inf, 1.5])
    v[0, 5, 1], v[0, 36, 3], v[3, 0, 0] = math.nan, math.inf, -math.inf
    v[1, 7, 2], v[1, 8, 0] = math.nan, math.inf
    out = _out(n * hw * 4, R.DT[prec])
    G.lib.jck_gp_grad(prec, _dev(v, prec), nr.cuda(), COEF, n, hw, out, G.cur_stream())
    got = _take(out, n * hw * 4, "gp_grad").view(n, hw, 4).float()
    bad = ~torch.isfinite(v)
    for img in (0, 3):                              # finite norm: non-finite exactly where g is, the rest as the reference
        assert torch.equal(~torch.isfinite(got[img]), bad[img])
        want = R.store(R.candidates_gp_grad(COEF, nr[img], v[img])[0]["one"], prec).float()
        assert torch.equal(got[img][~bad[img]], want[~bad[img]])
    assert math.isnan(got[0, 5, 1].item()) and got[0, 36, 3].item() == -math.inf and got[3, 0, 0].item() == -math.inf   # f < 0, > 0
    assert bool((got[1][~bad[1]] == 0).all()) and bool(torch.isnan(got[1][bad[1]]).all())      # NaN norm: f = 0
    assert bool(torch.isnan(got[2]).all())                                                      # infinite norm: f = NaN
    x = v.double().clone().requires_grad_(True)
    (COEF / 2 * ((torch.linalg.vector_norm(x.reshape(n, -1), dim=1) - 1) ** 2).sum()).backward()
    assert bool(torch.isnan(x.grad[0]).all()) and bool(torch.isnan(x.grad[1]).all()) and bool(torch.isnan(x.grad[3]).all())


# ---- img_prep_u8 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather", [True, False], ids=["idx", "first"])
@pytest.mark.parametrize("hw", R.U8_SHAPES, ids=_ids)
def test_img_prep_u8(G, hw, gather):
    """out_nchw bit for bit up2_pil_ref (one-pixel-wide and -high sources: both clamped taps are the pixel itself; Hs != Ws), and
    out_nhwc4 = rn_T(fma(mix, noise, rn(keep * t))) with lane 3 = +0, in both storage types, from one launch that writes both and
    from launches that write one; a batch of 4 gathered through idx = [3, 0, 3, 1] out of 5 images, and idx = NULL"""
    hs, ws = hw
    b, px = 4, 4 * hs * ws
    data, noise = R.make_u8(hs, ws)
    idx = R.U8_IDX if gather else None
    t = R.up2_pil_ref(data if gather else data[:b], idx)
    want, sums = R.expected_img_prep(KEEP, MIX, t.flatten(2), noise.flatten(2))
    assert R.ambiguous_count(sums) == 0
    ddata, dnoise = data.cuda(), noise.cuda()
    didx = torch.tensor(idx, dtype=torch.int64, device="cuda") if gather else None
    for prec in PRECS:
        for both in (True, False):
            o4, oc = _out(b * px * 4, R.DT[prec]), _out(b * 3 * px, torch.float32)
            if both:
                G.lib.jck_img_prep_u8(prec, ddata, didx, dnoise, KEEP, MIX, o4, oc, b, hs, ws, G.cur_stream())
            else:
                G.lib.jck_img_prep_u8(prec, ddata, didx, dnoise, KEEP, MIX, o4, None, b, hs, ws, G.cur_stream())
                G.lib.jck_img_prep_u8(prec, ddata, didx, None, 1.0, 0.0, None, oc, b, hs, ws, G.cur_stream())
            got4 = _take(o4, b * px * 4, "img_prep_u8 nhwc4").view(b, px, 4)
            gotc = _take(oc, b * 3 * px, "img_prep_u8 nchw").view(b, 3, 2 * hs, 2 * ws)
            assert torch.equal(R.bits(gotc), R.bits(t)), f"img_prep_u8 {hw} prec {prec}: out_nchw"
            _assert_same(got4, want, prec, f"img_prep_u8 {hw} prec {prec}: out_nhwc4")
            _lane3_zero(got4, "img_prep_u8")


def test_img_prep_u8_arguments(G):
    """both outputs NULL: OK and nothing to launch; B < 1, a NULL dataset, Hs or Ws < 1: JckError, nothing written"""
    data, noise = R.make_u8(5, 9)
    ddata, dnoise = data.cuda(), noise.cuda()
    st = G.cur_stream()
    assert G.lib.jck_img_prep_u8(1, ddata, None, dnoise, KEEP, MIX, None, None, 4, 5, 9, st) == 0
    o4, oc = _out(4 * 180 * 4, torch.float32, 5.0), _out(4 * 3 * 180, torch.float32, 6.0)
    for what, args in (("B = 0", (ddata, 0, 5, 9)), ("B = -1", (ddata, -1, 5, 9)), ("no data", (None, 4, 5, 9)), ("Hs = 0", (ddata, 4, 0, 9)),
                       ("Ws = 0", (ddata, 4, 5, 0))):
        d, b, hs, ws = args
        _raises_and_leaves(G, lambda: G.lib.jck_img_prep_u8(1, d, None, dnoise, KEEP, MIX, o4, oc, b, hs, ws, st), [o4, oc], f"img_prep_u8 {what}")


# ---- bf16x3 stores fp32 -----------------------------------------------------------------------------------------------------------
def test_bf16x3_gives_the_fp32_bits(G):
    """prec = 2 (fp32 storage, split-bf16 GEMMs) runs the fp32 instantiation of every kernel here: the bits of prec = 1 at (5, 37)"""
    n, hw = 5, 37
    num = n * hw * 4
    st = G.cur_stream()
    img, nz = R.make_img_prep(n, hw)
    x, nz2 = R.make_axpy(n, hw, 1)
    a, b, al = R.make_interp(n, hw, 1)
    tg, ty = R.make_tanh_bwd(n, hw, 1)
    gv, nr = R.make_gp_grad(n, hw, 1)
    data, noise = R.make_u8(5, 9)
    dimg, dnz, dx, dnz2, da, db, dal, dtg, dty, dgv, dnr, ddata, dnoise = (t.cuda() for t in (img, nz, x, nz2, a, b, al, tg, ty, gv, nr, data, noise))
    res = {}
    for prec in (1, 2):
        o = {k: _out(num, torch.float32) for k in ("img_prep", "axpy", "interp", "mix_out", "mix_xhat", "tanh_bwd", "gp_grad")}
        o["nchw"], o["norms"], o["scal"] = _out(n * 3 * hw, torch.float32), _out(n, torch.float32), _out(8 * n, torch.float32)
        o["u8_4"], o["u8_c"] = _out(4 * 180 * 4, torch.float32), _out(4 * 3 * 180, torch.float32)
        G.lib.jck_img_prep(prec, dimg, dnz, KEEP, MIX, o["img_prep"], n, hw, st)
        G.lib.jck_axpy_noise(prec, dx, dnz2, KEEP, MIX, o["axpy"], n, hw, st)
        G.lib.jck_interp(prec, da, db, dal, o["interp"], n, hw, st)
        G.lib.jck_mix_interp(prec, dx, dnz2, None, 0, KEEP, MIX, o["mix_out"], da, dal, o["mix_xhat"], n, hw, st)
        G.lib.jck_nhwc4_to_nchw(prec, da, o["nchw"], n, hw, st)
        G.lib.jck_tanh_bwd(prec, dtg, dty, KEEP, o["tanh_bwd"], num, st)
        G.lib.jck_gp_norm(prec, dgv, n, hw, o["scal"], 6, n, o["norms"], st)
        G.lib.jck_gp_grad(prec, dgv, dnr, COEF, n, hw, o["gp_grad"], st)
        G.lib.jck_img_prep_u8(prec, ddata, None, dnoise, KEEP, MIX, o["u8_4"], o["u8_c"], 4, 5, 9, st)
        torch.cuda.synchronize()
        res[prec] = o
    for k in res[1]:
        assert torch.equal(R.bits(res[1][k]), R.bits(res[2][k])), k
        assert not bool(torch.isnan(res[1][k][:-GUARD]).all()), f"{k}: never written"
    from hipgan._lib import JckError
    with pytest.raises(JckError):
        G.lib.jck_interp(3, da, db, dal, res[1]["interp"], n, hw, st)
