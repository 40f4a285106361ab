"""The metric-network kernels (csrc/infer.hip) one by one against plain torch / numpy on the CPU: exact where there is one right
answer, and with non-finite inputs.  Every number the project judges training by (Inception Score, FID) goes through them.

1. Convolution on integer data, bit for bit.  Activations and weights are integers in [-2, 2] (weights drawn independently per
   (kh, kw, ci, co): a transposed tap, swapped kh / kw or a wrong ci wrap cannot cancel), scale is 0.5 / 1 / 2, shift an integer
   in [-3, 3].  Every partial sum is an integer of magnitude <= 4 K < 2^24 (asserted per case), so the fp32 MFMA chain and the
   epilogue - fused or not - are exact and torch.equal against fp64 F.conv2d must hold.  Each case runs with ReLU on and off
   and with scale as a tensor and as None, into a channel slice of a wider tensor whose other channels keep a sentinel.
2. The two convolution kernels on seeded randn data: every case the c16 kernel serves runs once as dispatched and once with x
   as a view 4 bytes into a larger buffer, which fails the launcher's alignment test and takes the generic kernel.  The two
   outputs are compared as bit patterns (the claim in the comment above conv2d_nhwc_f32_c16_kernel); the aligned one stays inside
   tests/test_inception_gpu.py's bound against fp32 F.conv2d, 2e-5 * max(1, |ref|.max()).
3. Pools, layout change, global average: torch.equal (average pools on integers in [-8, 8]: the sums are exact and v / 9.f is
   a correctly rounded division), including one case per kernel above the 16384 * 256-thread grid cap, where the grid-stride
   loop takes its second trip.
4. NaN, +inf and -inf in the input come out where, and as what, torch on the CPU puts them - per kernel and through the whole
   chain (one NaN pixel: that image's logits, the feature mean / covariance and the FID are NaN; the other images' logits do not
   change by a bit).
5. The chain's logits do not depend on the chunking (which images share a tile).
6. jck_mean_cov_f64 against numpy in fp64 with a bound derived from the data, |cov - ref| <= 4 N 2^-52 (|xc|^T |xc|) / (N - 1)
   elementwise (xc the centred data; the mean likewise with |x|): N u sum|terms| is the worst case of ANY summation order of N
   fp64 terms, once for the kernel and once for numpy, and the factor 4 leaves room for the rounding of the centring and of
   the products.  N below / at / above the 256-thread stride, N = 1 and 2, D = 1, an ill-conditioned column.
7. Refused arguments raise and leave the output untouched (refused before any launch).
"""
import contextlib
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = -777.25                     # no integer-data result can be this (they are multiples of 0.5), nor a pooled integer / 9
GRID_CAP = 16384 * 256             # infer.hip grid1d(): above this many elements a thread loops
NAN, INF = float("nan"), float("inf")

# (N, H, W, Cin, Cout, (KH, KW), (SH, SW), (PH, PW))
GENERIC = {                                                          # Cin % 16 != 0 or Cout % 4 != 0
    "stem_k27": (2, 29, 31, 3, 32, (3, 3), (2, 2), (0, 0)),          # K = 27: no multiple of 16
    "one_channel_m25": (1, 5, 5, 3, 1, (3, 3), (1, 1), (1, 1)),
    "cout66_k119": (1, 9, 7, 17, 66, (1, 7), (1, 1), (0, 3)),        # Cout crosses a 64 tile
    "cin16_cout6": (3, 8, 8, 16, 6, (1, 1), (1, 1), (0, 0)),         # generic only because Cout % 4 != 0
    "m64": (1, 8, 8, 5, 7, (1, 1), (1, 1), (0, 0)),
    "m65": (1, 5, 13, 5, 7, (1, 1), (1, 1), (0, 0)),
}
C16 = {                                                              # Cin % 16 == 0, Cout % 4 == 0, aligned pointers
    "m1_nk1_cout4": (1, 1, 1, 16, 4, (1, 1), (1, 1), (0, 0)),        # the pipeline prologue is the whole loop
    "m127_cout60": (1, 1, 127, 16, 60, (1, 1), (1, 1), (0, 0)),
    "m128_nk2_cout64": (1, 8, 16, 32, 64, (1, 1), (1, 1), (0, 0)),
    "m129_cout68": (1, 3, 43, 16, 68, (1, 1), (1, 1), (0, 0)),
    "fc_n1": (1, 1, 1, 2048, 100, (1, 1), (1, 1), (0, 0)),
    "fc_n5": (5, 1, 1, 2048, 100, (1, 1), (1, 1), (0, 0)),
    "k7x1_cin16": (1, 9, 6, 16, 16, (7, 1), (1, 1), (3, 0)),         # the tap changes on every k-step
    "k1x7_cin32": (2, 5, 11, 32, 20, (1, 7), (1, 1), (0, 3)),
    "k1x3": (1, 6, 9, 16, 36, (1, 3), (1, 1), (0, 1)),
    "k3x1": (1, 9, 6, 32, 12, (3, 1), (1, 1), (1, 0)),
    "k3x3_p1_cin32": (1, 7, 10, 32, 24, (3, 3), (1, 1), (1, 1)),     # the channel offset wraps every second step
    "k5x5_p2_cin48": (1, 9, 12, 48, 64, (5, 5), (1, 1), (2, 2)),
    "s2_35_to_17": (1, 35, 35, 16, 32, (3, 3), (2, 2), (0, 0)),
    "s2_8_to_3": (1, 8, 8, 32, 16, (3, 3), (2, 2), (0, 0)),          # the last row and column are never read
    "n3_hw49": (3, 7, 7, 64, 32, (1, 1), (1, 1), (0, 0)),            # one 128-pixel tile spans three images
    "full_width": (2, 35, 35, 288, 384, (3, 3), (2, 2), (0, 0)),
}
ALL = {**GENERIC, **C16}


def _api():
    from hipgan import lib
    from hipgan._lib import cur_stream
    return lib, cur_stream


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().float()


def _kc(wt):
    """[co][ci][kh][kw] -> [(kh, kw, ci)][co], the library's weight layout"""
    return wt.permute(2, 3, 1, 0).reshape(-1, wt.shape[0]).contiguous().float()


def _off_by_4_bytes(x):
    """the same values as a contiguous device view that starts 4 bytes into a larger buffer: not 16-byte aligned"""
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + 4 and v.data_ptr() % 16 == 4
    return v


def _conv(dims, x_dev, wk_dev, scale, shift, relu, left=8, right=24):
    """jck_conv2d_nhwc_f32 into channels [left, left + Cout) of a sentinel-filled tensor -> the slice (CPU, NHWC)"""
    lib, cur_stream = _api()
    n, h, w, cin, cout, k, s, p = dims
    oh, ow = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
    total = left + cout + right
    out = torch.full((n, oh, ow, total), SENT, device="cuda")
    lib.jck_conv2d_nhwc_f32(x_dev, wk_dev, None if scale is None else scale.float().cuda(), shift.float().cuda(), out, n, h, w, cin,
                            k[0], k[1], s[0], s[1], p[0], p[1], cout, total, left, relu, cur_stream())
    o = out.cpu()
    assert bool((o[..., :left] == SENT).all()) and bool((o[..., left + cout:] == SENT).all()), "wrote outside its channel slice"
    return o[..., left:left + cout]


def _epilogue(acc64, scale, shift, relu):
    """fp64 NCHW accumulators -> the expected output (fp32, NHWC)"""
    y = acc64 if scale is None else acc64 * scale.double().view(1, -1, 1, 1)
    y = y + shift.double().view(1, -1, 1, 1)
    return _nhwc(F.relu(y) if relu else y)


@functools.lru_cache(maxsize=None)
def _int_case(name):
    """seeded integer data of a case and its fp64 accumulators, computed once"""
    n, h, w, cin, cout, k, s, p = ALL[name]
    g = _gen(name)
    x = torch.randint(-2, 3, (n, cin, h, w), generator=g).double()
    wt = torch.randint(-2, 3, (cout, cin, k[0], k[1]), generator=g).double()
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)]
    shift = torch.randint(-3, 4, (cout,), generator=g).float()
    if name.startswith("fc"):
        shift = -1.0 - torch.randint(0, 3, (cout,), generator=g).float()       # a negative bias: negative logits must survive
    assert 2 * (4 * cin * k[0] * k[1]) + 3 < 2 ** 24                           # |any partial sum|, scaled and shifted: exact in fp32
    return x, wt, scale, shift, F.conv2d(x, wt, None, s, p)


# ---- 1. integer data, bit-exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL))
def test_conv_integer_data_is_bit_exact(name):
    x, wt, scale, shift, acc = _int_case(name)
    xd, wk = _nhwc(x).cuda(), _kc(wt).cuda()
    assert xd.data_ptr() % 16 == 0 and wk.data_ptr() % 16 == 0                 # a C16 case is dispatched to the c16 kernel
    for relu in (1, 0):
        for sc in (scale, None):
            ref = _epilogue(acc, sc, shift, relu)
            if not relu and ref.numel() >= 100:                                # (the fc shapes included; m1 has four outputs)
                assert bool((ref < 0).any())                                   # negative outputs have to survive relu = 0
            got = _conv(ALL[name], xd, wk, sc, shift, relu)
            bad = (got != ref)
            assert torch.equal(got, ref), (name, relu, sc is not None, int(bad.sum()), bad.nonzero()[:4].tolist(),
                                           got[bad][:4].tolist(), ref[bad][:4].tolist())


# ---- 2. generic kernel == c16 kernel, bit for bit, on random data ------------------------------------------------------------
@pytest.mark.parametrize("name", list(C16))
def test_conv_kernels_agree_bitwise(name):
    from hipgan._lib import _arg
    n, h, w, cin, cout, k, s, p = dims = C16[name]
    g = _gen("randn " + name)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k[0], k[1], generator=g) * (2.0 / (cin * k[0] * k[1])) ** 0.5
    fc = name.startswith("fc")                                                 # the chain's fc call: bias only, no ReLU
    scale = None if fc else 0.5 + torch.rand(cout, generator=g)
    shift = torch.randn(cout, generator=g) * 0.1
    relu = 0 if fc else 1
    ref = F.conv2d(x, wt, None, s, p)
    ref = (ref if fc else ref * scale.view(1, -1, 1, 1)) + shift.view(1, -1, 1, 1)
    ref = _nhwc(F.relu(ref) if relu else ref)
    xd, wk = _nhwc(x).cuda(), _kc(wt).cuda()
    assert xd.data_ptr() % 16 == 0 and wk.data_ptr() % 16 == 0                 # -> c16 kernel
    # -> generic kernel (scalar loads).  That rests on the launcher's own alignment term, not on the hardware, which takes an
    # unaligned 16-byte load: were the term dropped, both runs would be the c16 kernel and this comparison would hold vacuously.
    xv = _off_by_4_bytes(xd)
    assert _arg(xv) == xv.data_ptr()                                           # the binding passes the view's own address
    a = _conv(dims, xd, wk, scale, shift, relu)
    b = _conv(dims, xv, wk, scale, shift, relu)
    err, bound = (a - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item())
    diff = a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)
    print(f"{name}: c16 vs fp32 F.conv2d {err:.3e} (bound {bound:.3e}); elements that differ between the kernels {int(diff.sum())}")
    assert not bool(diff.any()), (name, int(diff.sum()), a[diff][:4].tolist(), b[diff][:4].tolist())
    assert err <= bound, (name, err, bound)


# ---- 3. pools, layout change, global average ---------------------------------------------------------------------------------
def _pool(x_nchw, k, s, p, mode, left=3, right=5):
    lib, cur_stream = _api()
    n, c, h, w = x_nchw.shape
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    total = left + c + right
    out = torch.full((n, oh, ow, total), SENT, device="cuda")
    lib.jck_pool2d_nhwc_f32(_nhwc(x_nchw).cuda(), out, n, h, w, c, k, s, p, mode, total, left, cur_stream())
    o = out.cpu()
    assert bool((o[..., :left] == SENT).all()) and bool((o[..., left + c:] == SENT).all()), "wrote outside its channel slice"
    return o[..., left:left + c]


def _same_with_non_finite(got, ref):
    """NaN where torch has NaN; everything else - infinities with their sign included - equal"""
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (int(torch.isnan(got).sum()), int(torch.isnan(ref).sum()))
    m = ~torch.isnan(ref)
    assert torch.equal(got[m], ref[m]), ((got[m] != ref[m]).sum().item(), got[m][got[m] != ref[m]][:4].tolist(),
                                         ref[m][got[m] != ref[m]][:4].tolist())


# max 3/2/0: 147 -> 73, 71 -> 35, 35 -> 17, 17 -> 8, 3 -> 1, non-square; 3/1/1 at more than GRID_CAP outputs (second loop trip)
@pytest.mark.parametrize("shape,k,s,p", [((1, 1, 147, 147), 3, 2, 0), ((1, 33, 71, 71), 3, 2, 0), ((2, 64, 35, 35), 3, 2, 0),
                                         ((2, 33, 17, 17), 3, 2, 0), ((3, 1, 3, 3), 3, 2, 0), ((2, 64, 9, 4), 3, 2, 0),
                                         ((4, 64, 147, 147), 3, 1, 1)])
def test_max_pool_is_exact(shape, k, s, p):
    x = torch.randn(*shape, generator=_gen(f"max{shape}"))
    ref = _nhwc(F.max_pool2d(x, k, s, p))
    if s == 1:
        assert ref.numel() > GRID_CAP
    assert torch.equal(_pool(x, k, s, p, 0), ref)


# avg 3/1/1 (count_include_pad): 35, 17, 8, 1x1, non-square; (4, 147, 147, 64) has more than GRID_CAP outputs
@pytest.mark.parametrize("shape", [(1, 64, 35, 35), (2, 33, 17, 17), (2, 1, 8, 8), (3, 33, 1, 1), (2, 64, 5, 12), (4, 64, 147, 147)])
def test_avg_pool_integer_data_is_exact(shape):
    x = torch.randint(-8, 9, shape, generator=_gen(f"avg{shape}")).float()
    ref = _nhwc(F.avg_pool2d(x.double(), 3, 1, 1))
    if shape[0] == 4:
        assert ref.numel() > GRID_CAP
    assert torch.equal(_pool(x, 3, 1, 1, 1), ref)


@pytest.mark.parametrize("shape", [(2, 3, 299, 299), (1, 1, 1, 1), (3, 5, 7, 2), (16, 3, 299, 299)])
def test_nchw_to_nhwc_is_a_permutation(shape):
    lib, cur_stream = _api()
    n, c, h, w = shape
    numel = n * c * h * w
    assert numel < 2 ** 24 and (n != 16 or numel > GRID_CAP)                    # every element distinct and exact in fp32
    x = torch.arange(numel, dtype=torch.float32).view(shape)
    out = torch.full((numel + 64,), SENT, device="cuda")
    lib.jck_nchw_to_nhwc_f32(x.cuda(), out, n, c, h, w, cur_stream())
    o = out.cpu()
    assert torch.equal(o[:numel].view(n, h, w, c), x.permute(0, 2, 3, 1))
    assert bool((o[numel:] == SENT).all())


# (N, HW, C): the chain's 8x8x2048, HW = 1, and N * C above GRID_CAP
@pytest.mark.parametrize("n,hw,c", [(3, 64, 2048), (2, 1, 2048), (2049, 1, 2048)])
def test_global_avgpool_integer_data_is_exact(n, hw, c):
    lib, cur_stream = _api()
    assert n != 2049 or n * c > GRID_CAP
    x = torch.randint(-8, 9, (n, hw, c), generator=_gen(f"gap{n},{hw},{c}")).float()
    out = torch.full((n * c + 64,), SENT, device="cuda")
    lib.jck_global_avgpool_nhwc_f32(x.cuda(), out, n, hw, c, cur_stream())
    o = out.cpu()
    assert torch.equal(o[:n * c].view(n, c), x.double().mean(1).float())
    assert bool((o[n * c:] == SENT).all())


# ---- 4. non-finite values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,misaligned", [("cout66_k119", False), ("stem_k27", False), ("k3x3_p1_cin32", False),
                                             ("k3x3_p1_cin32", True), ("s2_8_to_3", False), ("s2_8_to_3", True)])
def test_conv_propagates_non_finite_like_torch(name, misaligned):
    """One NaN, one +inf, one -inf, and a +inf / -inf pair in two channels of one pixel (inf - inf = NaN where both weights have
    the same sign, an infinity otherwise; inf * 0 = NaN where a weight is zero).  All of it is independent of the summation
    order, the finite part stays integer: one right answer per element.  Both kernels (a C16 case off alignment runs the generic)."""
    x, wt, scale, shift, _ = _int_case(name)
    n, c, h, w = x.shape
    x = x.clone()
    x[0, c // 2, h // 2, w // 2] = NAN
    x[0, 0, 0, 0] = INF
    x[n - 1, c - 1, h - 2, w - 2] = -INF
    x[n - 1, 0, h // 2, 1] = INF
    x[n - 1, c - 1, h // 2, 1] = -INF
    dims = ALL[name]
    acc = F.conv2d(x, wt, None, dims[6], dims[7])
    xd, wk = _nhwc(x).cuda(), _kc(wt).cuda()
    if misaligned:
        xd = _off_by_4_bytes(xd)
    for relu in (1, 0):
        ref = _epilogue(acc, scale, shift, relu)
        assert bool(torch.isnan(ref).any()) and bool((ref == INF).any()) and bool(torch.isfinite(ref).any())
        assert relu or bool((ref == -INF).any())
        _same_with_non_finite(_conv(dims, xd, wk, scale, shift, relu), ref)


def _pool_poison(shape, tag):
    x = torch.randint(-8, 9, shape, generator=_gen(tag)).float()
    x[0, 0, 0:3, 0:3] = -INF                       # a whole 3x3 window of -inf: its maximum is -inf
    x[0, 0, 5, 5] = NAN
    x[1, 1, 4, 4] = INF
    x[1, 1, 4, 6] = -INF                           # one column apart: the average windows that hold both are NaN
    x[1, 2, 8, 8] = -INF
    return x


def test_max_pool_propagates_non_finite_like_torch():
    x = _pool_poison((2, 3, 9, 9), "maxnf")
    ref = _nhwc(F.max_pool2d(x, 3, 2, 0))
    assert ref[0, 0, 0, 0] == -INF and int(torch.isnan(ref).sum()) == 1 and bool((ref == INF).any())
    _same_with_non_finite(_pool(x, 3, 2, 0, 0), ref)
    ref = _nhwc(F.max_pool2d(x, 3, 1, 1))           # overlapping windows: the NaN reaches nine outputs
    assert int(torch.isnan(ref).sum()) == 9
    _same_with_non_finite(_pool(x, 3, 1, 1, 0), ref)


def test_avg_pool_propagates_non_finite_like_torch():
    x = _pool_poison((2, 3, 9, 9), "avgnf")
    ref = _nhwc(F.avg_pool2d(x.double(), 3, 1, 1))
    assert int(torch.isnan(ref).sum()) > 9 and bool((ref == INF).any()) and bool((ref == -INF).any())
    _same_with_non_finite(_pool(x, 3, 1, 1, 1), ref)


def test_global_avgpool_propagates_non_finite_like_torch():
    lib, cur_stream = _api()
    n, hw, c = 2, 9, 8
    x = torch.randint(-8, 9, (n, hw, c), generator=_gen("gapnf")).float()
    x[0, 4, 1], x[0, 2, 3], x[1, 8, 5] = NAN, INF, -INF
    x[1, 0, 7], x[1, 5, 7] = INF, -INF
    ref = x.double().mean(1).float()
    assert int(torch.isnan(ref).sum()) == 2 and int(torch.isinf(ref).sum()) == 2
    out = torch.full((n, c), SENT, device="cuda")
    lib.jck_global_avgpool_nhwc_f32(x.cuda(), out, n, hw, c, cur_stream())
    # HW = 9: on finite integer columns sum / 9.f is the correctly rounded quotient, as the fp64 mean cast to fp32 is
    _same_with_non_finite(out.cpu(), ref)


@pytest.fixture(scope="module")
def net():
    from inception import InceptionV3Hip
    from oracle.inception_oracle import random_state_dict
    sd = random_state_dict(0)
    return sd, InceptionV3Hip(sd)


@contextlib.contextmanager
def _chunk(hip, chunk):
    """images per pass of the shared network for one block only: a failing assertion leaves the other tests' chunk as it was"""
    keep, hip.chunk = hip.chunk, chunk
    try:
        yield hip
    finally:
        hip.chunk = keep


def test_chain_one_nan_pixel_gives_nan_scores(net):
    """A diverged generator's NaN image must show in the scores: torch's network (the CPU restatement) returns NaN logits for it."""
    from metrics import fid_from_features, inception_score_from_probs, mean_cov
    from oracle.inception_oracle import inception_logits
    sd, hip = net
    x = torch.randn(3, 3, 299, 299, generator=_gen("chain nan"))
    bad = x.clone()
    bad[1, 1, 150, 150] = NAN
    assert bool(torch.isnan(inception_logits(sd, bad[1:2])).all())             # the reference arithmetic: every logit NaN
    with _chunk(hip, 64):                                                      # the three images share tiles
        clean, got = hip(x.cuda()).cpu(), hip(bad.cuda())
    assert bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(got[1]).all()), got[1].cpu()[:8].tolist()
    assert torch.equal(got[0].cpu(), clean[0]) and torch.equal(got[2].cpu(), clean[2])
    mu, cov = mean_cov(got)
    assert np.isnan(mu).all() and np.isnan(cov).all()
    real = torch.randn(50, 100, generator=_gen("real feats"))
    for r in (real.cuda(), real.numpy()):
        assert np.isnan(fid_from_features(r, got if torch.is_tensor(r) else got.cpu().numpy()))
    assert np.isnan(inception_score_from_probs(torch.softmax(got.cpu(), 1).numpy(), splits=1))


# ---- 5. batch independence ---------------------------------------------------------------------------------------------------
def test_chain_logits_do_not_depend_on_the_chunking(net):
    _, hip = net
    x = torch.randn(5, 3, 299, 299, generator=_gen("chunks")).cuda()
    outs = []
    for chunk in (1, 2, 5):
        with _chunk(hip, chunk):
            outs.append(hip(x).cpu())
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), ((outs[0] - outs[1]).abs().max().item(),
                                                                             (outs[0] - outs[2]).abs().max().item())


# ---- 6. fp64 mean / covariance -----------------------------------------------------------------------------------------------
def _mean_cov_case(x32, tag):
    from metrics import mean_cov_device
    x = x32.astype(np.float64)
    n, d = x.shape
    mu_ref, cov_ref = np.mean(x, axis=0), np.cov(x, rowvar=False).reshape(d, d)
    xc = np.abs(x - mu_ref)
    mu_bound = 4 * n * 2.0 ** -52 * np.abs(x).sum(axis=0) / n
    cov_bound = 4 * n * 2.0 ** -52 * (xc.T @ xc) / (n - 1)
    xd = torch.from_numpy(x32).cuda()
    mu, cov = mean_cov_device(xd)
    mu2, cov2 = mean_cov_device(xd)
    assert torch.equal(mu, mu2) and torch.equal(cov, cov2)                     # fixed summation order
    assert torch.equal(cov, cov.t())                                           # exactly symmetric
    mu, cov = mu.cpu().numpy(), cov.cpu().numpy()
    assert np.isfinite(mu).all() and np.isfinite(cov).all()
    r_mu, r_cov = (np.abs(mu - mu_ref) / mu_bound).max(), (np.abs(cov - cov_ref) / cov_bound).max()
    print(f"mean_cov {tag}: |mean err| / bound {r_mu:.3f}, |cov err| / bound {r_cov:.3f} (the bound holds the factor 4)")
    assert (np.abs(mu - mu_ref) <= mu_bound).all(), (tag, r_mu)
    assert (np.abs(cov - cov_ref) <= cov_bound).all(), (tag, r_cov)


@pytest.mark.parametrize("n,d", [(2, 3), (50, 100), (255, 7), (256, 7), (257, 7), (1000, 1), (64, 2048)])
def test_mean_cov_within_the_fp64_bound(n, d):
    rng = np.random.default_rng(1000 * n + d)
    _mean_cov_case((1.5 * rng.standard_normal((n, d)) + 0.2).astype(np.float32), f"({n}, {d})")


def test_mean_cov_ill_conditioned_column():
    """Mean 1e4, spread 1e-2 (ten fp32 steps): the two-pass form centres first and stays inside the same bound; a one-pass
    E[x^2] - E[x]^2 would be rounding 1e8-sized terms to get a 1e-4-sized variance."""
    rng = np.random.default_rng(5)
    _mean_cov_case((1e4 + 1e-2 * rng.standard_normal((500, 8))).astype(np.float32), "1e4 + 1e-2 randn (500, 8)")


def test_mean_cov_of_one_row():
    """The project's choice (infer.hip divides by N > 1 ? N - 1 : 1): one row gives its own values as the mean and an all-zero
    covariance.  numpy gives NaN there (0 / 0)."""
    from metrics import mean_cov_device
    x = torch.randn(1, 5, generator=_gen("one row"))
    mu, cov = mean_cov_device(x.cuda())
    assert torch.equal(mu.cpu(), x[0].double())
    assert torch.equal(cov.cpu(), torch.zeros(5, 5, dtype=torch.float64))


# ---- 7. refused arguments ----------------------------------------------------------------------------------------------------
def test_refused_arguments_raise_and_write_nothing():
    from hipgan._lib import JckError
    lib, cur_stream = _api()
    x = torch.ones(1, 4, 4, 16, device="cuda")
    wk = torch.ones(9 * 16, 8, device="cuda")
    out = torch.full((1, 4, 4, 16), SENT, device="cuda")
    with pytest.raises(JckError, match="outside the channel stride"):          # channels [12, 20) of 16
        lib.jck_conv2d_nhwc_f32(x, wk, None, None, out, 1, 4, 4, 16, 1, 1, 1, 1, 0, 0, 8, 16, 12, 1, cur_stream())
    with pytest.raises(JckError, match="outside the channel stride"):
        lib.jck_conv2d_nhwc_f32(x, wk, None, None, out, 1, 4, 4, 16, 1, 1, 1, 1, 0, 0, 8, 16, -1, 1, cur_stream())
    with pytest.raises(JckError, match="larger than the padded input"):        # 3x3 on a 2x2 input without padding
        lib.jck_conv2d_nhwc_f32(x, wk, None, None, out, 1, 2, 2, 16, 3, 3, 1, 1, 0, 0, 8, 16, 0, 1, cur_stream())
    with pytest.raises(JckError, match="larger than the padded input"):        # the same at stride 2, where (2 - 3) / 2 + 1 is 1 in C
        lib.jck_conv2d_nhwc_f32(x, wk, None, None, out, 1, 2, 2, 16, 3, 3, 2, 2, 0, 0, 8, 16, 0, 1, cur_stream())
    with pytest.raises(JckError, match="larger than the padded input"):        # one dimension fits, the other does not
        lib.jck_conv2d_nhwc_f32(x, wk, None, None, out, 1, 4, 2, 16, 3, 3, 2, 2, 0, 0, 8, 16, 0, 1, cur_stream())
    with pytest.raises(JckError, match="pool2d: bad arguments"):
        lib.jck_pool2d_nhwc_f32(x, out, 1, 4, 4, 16, 3, 1, 1, 2, 16, 0, cur_stream())
    with pytest.raises(JckError, match="pool2d: bad geometry"):                # slice past the channel stride; window too large
        lib.jck_pool2d_nhwc_f32(x, out, 1, 4, 4, 16, 3, 1, 1, 0, 16, 4, cur_stream())
    with pytest.raises(JckError, match="pool2d: bad geometry"):
        lib.jck_pool2d_nhwc_f32(x, out, 1, 2, 2, 16, 3, 2, 0, 0, 16, 0, cur_stream())
    with pytest.raises(JckError, match="pool2d: bad geometry"):
        lib.jck_pool2d_nhwc_f32(x, out, 1, 2, 2, 16, 3, 1, 0, 0, 16, 0, cur_stream())
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
