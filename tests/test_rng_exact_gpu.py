"""The Philox draws of a training step against tests/philox_ref.py (pinned on the CPU to the Random123 known answers):
jck_step_rng's alpha and masks bit for bit and its z to library-function accuracy, the image kernels' in-kernel noise against the
float64 pixel normals, and engine steps that draw for themselves against steps handed every draw from the per-op entry points."""
import numpy as np
import pytest
import torch

import philox_ref as P

pytestmark = pytest.mark.gpu

SEED_HI = (0x5eed1234 << 32) | 0x9abc0def          # a seed with a non-zero high word


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _step_rng(G, step, seed, nz, na, nm, keep_p, guard=8):
    """-> z, alpha, masks as float32 numpy arrays INCLUDING `guard` sentinel elements (7.0) behind each, and the hp block"""
    hp = torch.zeros(8, device="cuda")
    bufs = [torch.full((n + guard,), 7.0, device="cuda") for n in (nz, na, nm)]
    G.lib.jck_step_rng(hp, step, seed, bufs[0] if nz else None, nz, bufs[1] if na else None, na, bufs[2] if nm else None, nm, keep_p,
                       G.cur_stream())
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in bufs] + [hp.cpu()]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


Z_ULPS = 16.0


def _check_z(z, nz, step, seed):
    """|z - ref| <= 16 * 2^-24 * r of the float64 reference on the kernel's own float32 u and float32 angle, r the element's reference
    radius; equal where r = 0.  The library functions are built to the OpenCL single-precision limits: logf 3 ulp (halved by the
    square root: 1.5), sqrtf 3, sincosf 4, the product r * c half an ulp; -2.0f * log is exact - 9 ulp in all, below the 12 at which the
    factor would have to be re-derived, so it stands at 16 (no fast-math in hipgan/build.py)."""
    ref, r = P.z_ref(nz, step, seed)
    err = np.abs(z[:nz].astype(np.float64) - ref)
    lim = Z_ULPS * 2.0 ** -24 * r
    bad = err > lim
    assert not bad.any(), (int(bad.sum()), int(np.argmax(err - lim)), float((err / np.maximum(r, 1e-300)).max() * 2.0 ** 24))
    assert np.all(z[:nz][r == 0] == 0)
    return float((err / np.maximum(r, 2.0 ** -30)).max() * 2.0 ** 24)


@pytest.mark.parametrize("keep_p", [0.75, 0.3])
@pytest.mark.parametrize("seed", [99, SEED_HI])
def test_step_rng_is_the_reference(G, seed, keep_p):
    """alpha and masks bit for bit, z to 16 * 2^-24 * r, at counts with n % 4 = 0, 1, 2, 3 (the three tensors take turns), steps 1, 2 and
    70000; the sentinels behind every ragged end stay."""
    for step, (nz, na, nm) in ((1, (800, 9, 2050)), (2, (801, 10, 2051)), (70000, (803, 11, 2048)), (3, (2, 8, 1))):
        z, a, m, hp = _step_rng(G, step, seed, nz, na, nm, keep_p)
        assert hp.view(torch.int32)[4:8].tolist() == [x - (1 << 32) if x >= 1 << 31 else x for x in (seed & 0xffffffff, seed >> 32, step, 0)]
        assert np.array_equal(_bits(a[:na]), _bits(P.alpha_ref(na, step, seed))), (step, "alpha")
        assert np.array_equal(_bits(m[:nm]), _bits(P.masks_ref(nm, step, seed, keep_p))), (step, "masks")
        _check_z(z, nz, step, seed)
        for buf, n in ((z, nz), (a, na), (m, nm)):
            assert np.all(buf[n:] == 7.0), (step, n)


def test_step_rng_past_the_grid_cap(G):
    """(nz + 3) / 4 + (nalpha + 3) / 4 + (nmask + 3) / 4 > 1024 * 256 quads: adam_hp_kernel's 1024 workgroups stride twice over the
    masks - a counter taken from a wrapped or workgroup-local index shows here."""
    nz, na, nm = 13, 6, 4 * 1024 * 256 + 51_427
    assert (nz + 3) // 4 + (na + 3) // 4 + (nm + 3) // 4 > 1024 * 256
    z, a, m, _ = _step_rng(G, 4, SEED_HI, nz, na, nm, 0.75)
    assert np.array_equal(_bits(m[:nm]), _bits(P.masks_ref(nm, 4, SEED_HI, 0.75)))
    assert np.array_equal(_bits(a[:na]), _bits(P.alpha_ref(na, 4, SEED_HI)))
    _check_z(z, nz, 4, SEED_HI)
    assert np.all(m[nm:] == 7.0) and np.all(a[na:] == 7.0) and np.all(z[nz:] == 7.0)


# ---- in-kernel image noise -----------------------------------------------------------------------------------------------------
# max |got - ref| / max(r, 2^-12) of the three pixel normals against the float64 reference, as measured on an MI355X over every draw
# of the tests below (v_log_f32, v_sqrt_f32, v_sin_f32, v_cos_f32 - hardware transcendentals with no documented error here); the
# tests assert 4 x this (other seeds may hit worse arguments), which must stay below 2^-12: every mapping error (a swapped word, sin
# for cos, a wrong tensor id, a local pixel index) moves most elements by O(0.1).
# Measured: 2.19e-7 (ids 0 and 1, 64x64), 1.89e-7 (16x16), 2.54e-7 = 2^-21.9 over the 2.1 M pixels past the grid cap - the same in
# all four kernels, which agree bit for bit.  Far below 2^-14: the hardware functions cost about four float32 ulps of the radius.
PIXEL_ERR_MEASURED = 2.54e-7
PIXEL_ERR_BOUND = 4.0 * PIXEL_ERR_MEASURED          # 1.02e-6 = 2^-19.9


def _rng_words(seed, step):
    w = torch.tensor([seed & 0xffffffff, seed >> 32, step, 0], dtype=torch.int64)
    return w.to(torch.int32).cuda()                 # the uint32 words, two's complement


def _check_pixels(out, npix, tensor_id, step, seed, what):
    """out: [npix, 4] float32 NHWC4 rows of a zero image mixed with weight 1: channels 0..2 are the normals, channel 3 is +0"""
    assert PIXEL_ERR_BOUND < 2.0 ** -12
    got = out.reshape(npix, 4).cpu().numpy()
    ref, r = P.pixel_normals_ref(npix, tensor_id, step, seed)
    assert np.all(_bits(got[:, 3]) == 0), what
    fig = float((np.abs(got[:, :3].astype(np.float64) - ref) / np.maximum(r, 2.0 ** -12)).max())
    print(f"pixel-normal error {what}: {fig:.4e} = 2^{np.log2(max(fig, 1e-300)):.2f}")
    assert fig <= PIXEL_ERR_BOUND, (what, fig, PIXEL_ERR_BOUND)
    return fig


@pytest.mark.parametrize("side", [16, 64])
@pytest.mark.parametrize("tensor_id", [0, 1])
def test_image_noise_is_the_reference(G, tensor_id, side):
    """jck_img_prep_rng, jck_axpy_noise_rng, jck_img_prep_u8_rng (and, at 64x64 - the any-size kernel makes 64 or 128 only -
    jck_img_prep_u8_any): N = 3 zero images (uint8 forms: keep = 0), mix = 1, fp32 storage: every pixel's three values against the
    float64 pixel normals of the GLOBAL pixel index n * HW + px, channel 3 exactly 0.
    Measured on the MI355X: max |got - ref| / max(r, 2^-12) = 2.19e-7 here (2.54e-7 over all draws of this module); asserted at
    4 x 2.54e-7 = 1.02e-6 (PIXEL_ERR_BOUND), below the 2^-12 = 2.4e-4 it must stay under."""
    n, hw, step, seed = 3, side * side, 5, SEED_HI
    rng = _rng_words(seed, step)
    st = G.cur_stream()
    outs = {k: torch.full((n, side, side, 4), 7.0, device="cuda") for k in ("img_prep", "axpy", "u8")}
    G.lib.jck_img_prep_rng(G.PREC_F32, torch.zeros(n, 3, side, side, device="cuda"), rng, tensor_id, 0.9, 1.0, outs["img_prep"], n, hw, st)
    G.lib.jck_axpy_noise_rng(G.PREC_F32, torch.zeros(n, side, side, 4, device="cuda"), rng, tensor_id, 0.37, 1.0, outs["axpy"], n, hw, st)
    data = torch.full((n, 3, side // 2, side // 2), 127, dtype=torch.uint8, device="cuda")
    G.lib.jck_img_prep_u8_rng(G.PREC_F32, data, None, rng, tensor_id, 0.0, 1.0, outs["u8"], n, side // 2, side // 2, st)
    if side == 64:
        from hipgan.engine import resize_taps
        outs["u8_any"] = torch.full((n, side, side, 4), 7.0, device="cuda")
        src = torch.full((n, 3, 20, 27), 200, dtype=torch.uint8, device="cuda")
        G.lib.jck_img_prep_u8_any(G.PREC_F32, src, None, None, None, rng, tensor_id, 0.0, 1.0, outs["u8_any"], None, n, 20, 27, 64,
                                  resize_taps(20, 27, 64, "cuda"), st)
    torch.cuda.synchronize()
    for k, o in outs.items():
        _check_pixels(o, n * hw, tensor_id, step, seed, f"{k} id {tensor_id} {side}x{side}")
    for k in outs:                                   # one mapping: the four kernels agree bit for bit
        assert torch.equal(outs[k], outs["img_prep"]), k


def test_image_noise_past_the_grid_cap(G):
    """N * HW = 513 * 4096 pixels > 8192 workgroups * 256 threads (ew_grid's cap at jck_img_prep_u8_rng's launch site): the stride
    loop wraps; 34 MB of output from a 1.6 MB uint8 batch.  Compared like the small cases (measured: 2.54e-7, the module's worst)."""
    n, hw, step, seed = 513, 64 * 64, 2, 31337
    assert n * hw > 8192 * 256
    out = torch.empty(n, 64, 64, 4, device="cuda")
    data = torch.full((n, 3, 32, 32), 127, dtype=torch.uint8, device="cuda")
    G.lib.jck_img_prep_u8_rng(G.PREC_F32, data, None, _rng_words(seed, step), 1, 0.0, 1.0, out, n, 32, 32, G.cur_stream())
    torch.cuda.synchronize()
    _check_pixels(out, n * hw, 1, step, seed, "u8 past the grid cap")


# ---- the step draws what the per-op entry points draw ---------------------------------------------------------------------------
def _handed_draws(G, family, B, step, seed, labels):
    """every draw of optimiser step `step` from the per-op entry points, with the counts jck_engine_set_step passes"""
    hp = torch.zeros(8, device="cuda")
    z, alpha = torch.empty(B * 100, device="cuda"), torch.empty(B, device="cuda")
    masks = torch.empty(4, B, 256, device="cuda") if family == "cgan" else None
    G.lib.jck_step_rng(hp, step, seed, z, B * 100, alpha, B, masks, 4 * B * 256 if masks is not None else 0, 0.75, G.cur_stream())
    rng = _rng_words(seed, step)
    zero = torch.zeros(B, 3, 64, 64, device="cuda")
    noise = {"z": z.view(B, 100, 1, 1), "alpha": alpha.view(B, 1, 1, 1)}
    for name, tensor_id in (("n1", 0), ("n2", 1)):
        o = torch.empty(B, 64, 64, 4, device="cuda")
        G.lib.jck_img_prep_rng(G.PREC_F32, zero, rng, tensor_id, 0.9, 1.0, o, B, 64 * 64, G.cur_stream())
        noise[name] = o[..., :3].permute(0, 3, 1, 2).contiguous()
    if family == "cgan":
        noise["labels"] = labels
        for i in range(4):
            noise[f"m{i + 1}"] = masks[i]
    return noise


@pytest.mark.parametrize("family,prec", [("dcgan", "f32"), ("dcgan", "bf16"), ("cgan", "bf16")])
def test_a_step_draws_what_the_entry_points_draw(G, family, prec):
    """Three eager batch-8 steps with noise=None (the set-step launch and the image kernels draw) and three with z, alpha, the four
    masks (one [4, B, 256] draw, keep 0.75) from jck_step_rng(step = t, seed) and n1 / n2 from jck_img_prep_rng on a zero image with
    tensor ids 0 / 1 and words {seed lo, seed hi, t, 0}: arenas, scalars and the fake batch bit for bit.  A step that used another
    tensor id, step word, seed word or operand row for one of its draws differs."""
    import bf16_error as be
    from hipgan.engine import CganEngine, DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    B, seed = 8, SEED_HI
    torch.manual_seed(12345)
    g, d = build_params(family)
    imgs = synth_images(B * 3)
    runs = []
    for handed in (False, True):
        eng = (CganEngine if family == "cgan" else DcganEngine)(batch=B, prec=prec)
        eng.load_state(g, d)
        eng.set_noise_seed(seed)
        sc = []
        for s in range(3):
            lab = be.labels_for(B, 5 + s).cuda() if family == "cgan" else None
            real = imgs[s * B:(s + 1) * B].cuda()
            if handed:
                eng.step_async(real, _handed_draws(G, family, B, s + 1, seed, lab), 2e-4)
            else:
                eng.step_async(real, None, 2e-4, labels=lab)
            sc.append(eng.scalars())
        torch.cuda.synchronize()
        runs.append((sc, {k: v.clone() for k, v in eng.arenas.items()}, eng.tensor("fake").clone()))
    (s0, a0, f0), (s1, a1, f1) = runs
    assert all(np.isfinite(list(x.values())).all() for x in s0)
    assert s0 == s1, (s0, s1)
    assert torch.equal(f0.view(torch.int16 if prec == "bf16" else torch.int32), f1.view(torch.int16 if prec == "bf16" else torch.int32))
    for k in a0:
        assert torch.equal(a0[k], a1[k]), k
