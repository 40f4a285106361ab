"""What tests/test_bn2_gpu.py rests on, checked on the CPU: (a) the closed form of tests/bn_ref.py is the second backward of
BatchNorm + activation (fp64 autograd), (b) with the inputs of bn_ref.inputs every term of it is far above the bf16 tolerance at
every shape the GPU test runs, (c) the rounding the kernels are entitled to - fp32 arithmetic, storage-type inputs and outputs -
stays within half of every tolerance of the GPU test.  Runs none of the HIP code."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref

SENSITIVITY = 3.0       # a dropped term must move its output by this many bf16 tolerances, relative to the maximum
OUTPUT_KEYS = ("u", "xdir", "uy")


def relmax(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-300))


@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("shape", [(37, 8), (700, 64)])
def test_closed_form_is_the_autograd_double_backward(shape, slope):
    """S = <v, gy> + <ua, a> with gy = autograd.grad(a, y, ga, create_graph=True):  dS/dga = u, dS/dy = uy,
    dS/dgamma = dgamma_vchain + dgamma_rev, dS/dbeta = dbeta_rev, each to 1e-12 of the maximum."""
    rows, C = shape
    inp = bn_ref.inputs(rows, C, seed=3)
    y, ga, gamma, beta = (inp[k].clone().requires_grad_(True) for k in ("y", "ga", "gamma", "beta"))
    v, ua = inp["v"], inp["ua"]
    bn = F.batch_norm(y, None, None, gamma, beta, True, 0.1, bn_ref.EPS)
    a = F.leaky_relu(bn, slope) if slope else F.relu(bn)
    gy, = torch.autograd.grad(a, y, ga, create_graph=True)
    S = (v * gy).sum() + (ua * a).sum()
    d_ga, d_y, d_gamma, d_beta = torch.autograd.grad(S, (ga, y, gamma, beta))
    ref = bn_ref.second_order(inp["y"], inp["ga"], v, ua, inp["gamma"], inp["beta"], slope)
    first = bn_ref.first_order(inp["y"], inp["ga"], inp["gamma"], inp["beta"], slope)
    assert relmax(first["a"], a.detach()) <= 1e-12
    assert relmax(first["gy"], gy.detach()) <= 1e-12
    assert relmax(ref["u"], d_ga) <= 1e-12
    assert relmax(ref["uy"], d_y) <= 1e-12
    assert relmax(ref["dgamma_vchain"] + ref["dgamma_rev"], d_gamma) <= 1e-12
    assert relmax(ref["dbeta_rev"], d_beta) <= 1e-12
    # the first backward's parameter gradients and statistics
    gm, bt = inp["gamma"].clone().requires_grad_(True), inp["beta"].clone().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    bn = F.batch_norm(inp["y"], rm, rv, gm, bt, True, 1.0, bn_ref.EPS)
    (F.leaky_relu(bn, slope) if slope else F.relu(bn)).backward(inp["ga"])
    assert relmax(first["dgamma"], gm.grad) <= 1e-12 and relmax(first["dbeta"], bt.grad) <= 1e-12
    assert relmax(first["mean"], rm) <= 1e-12 and relmax(first["unbiased"], rv) <= 1e-12
    assert relmax(first["var"], inp["y"].var(0, unbiased=False)) <= 1e-12


@pytest.mark.parametrize("shape", bn_ref.SHAPES)
def test_every_term_is_visible_in_bf16(shape):
    """Leaving out any one term of the closed form moves the output it belongs to by at least 3x the GPU test's bf16 tolerance
    (relative to the maximum), with ua ~ N(0,1) or with ua = 0: a kernel that lost the term fails tests/test_bn2_gpu.py in
    either storage type."""
    rows, C = shape
    need = SENSITIVITY * bn_ref.TOL["bf16"]["tensor"]
    moved = {t: 0.0 for t in bn_ref.TERMS}
    for kind in bn_ref.UA_KINDS:
        inp = bn_ref.inputs(rows, C, seed=0, kind=kind)
        full = bn_ref.second_order(slope=0.2, **inp)
        for term, out in bn_ref.TERMS.items():
            if kind == "zero" and out != "uy":
                continue                                    # u and xdir do not depend on ua
            part = bn_ref.second_order(slope=0.2, drop=term, **inp)
            for k in OUTPUT_KEYS:
                if k != out and not (k == "uy" and out == "xdir"):      # uy reads xdir
                    assert torch.equal(part[k], full[k]), (term, k)
            moved[term] = max(moved[term], relmax(part[out], full[out]))
    print(f"{shape}: " + ", ".join(f"{t} {m:.3f}" for t, m in moved.items()))
    for term, m in moved.items():
        assert m >= need, f"{shape}: dropping {term} moves {bn_ref.TERMS[term]} by {m:.3e} of its maximum < {need:.1e}"


def emulate(inp, slope, bf16):
    """The chain as the kernels run it (csrc/bn.hpp, csrc/bn2.hpp), in fp32 on the CPU: statistics rows rounded once from fp64, finalize in double,
    everything else in fp32; y, ga, v, ua arrive in the storage type and gy, xdir, u, uy are rounded to it where the kernels store
    them.  The sums are torch's fp32 sums: the order of a summation is the kernels' own business."""
    st = (lambda t: t.float().bfloat16().float()) if bf16 else (lambda t: t.float())
    y, ga, v, ua = (st(inp[k]) for k in ("y", "ga", "v", "ua"))
    gamma, beta = inp["gamma"].float(), inp["beta"].float()
    n = y.shape[0]
    s, q = y.double().sum(0).float(), (y.double() ** 2).sum(0).float()
    meand = s.double() / n
    vard = (q.double() / n - meand * meand).clamp_min(0.0)
    mean, var = meand.float(), vard.float()
    invstd = 1.0 / torch.sqrt(var + torch.tensor(bn_ref.EPS, dtype=torch.float32))
    sc = gamma * invstd
    sh = beta - mean * sc
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    pos = y * sc + sh > 0
    act = lambda t: torch.where(pos, t, slope * t)
    xh = (y - mean) * invstd
    gz = act(ga)
    s1a, s1b = gz.sum(0), (gz * xh).sum(0)
    gy = st(sc * (gz - s1a * inv - xh * (s1b * inv)))
    # v-chain
    sv, svx, svgy = v.sum(0), (v * xh).sum(0), (v * gy).sum(0)
    m1, m2, mv, mvx = s1a * inv, s1b * inv, sv * inv, svx * inv
    gz2 = gy / sc + m1 + xh * m2
    xdir = st(-sc * (v * m2 + gz2 * mvx))
    u = st(act(sc * (v - mv - xh * mvx)))
    # reverse sweep
    uz = act(ua)
    suz, suzx, sxd, sxdx = uz.sum(0), (uz * xh).sum(0), xdir.sum(0), (xdir * xh).sum(0)
    qq = gamma * uz + xdir
    mq, mqx = (gamma * suz + sxd) * inv, (gamma * suzx + sxdx) * inv
    uy = st((qq - mq - xh * mqx) * invstd - svgy * invstd * xh * inv)
    for t in (gy, xdir, u, uy, sv, suz):
        assert t.dtype == torch.float32
    rounded = dict(inp, y=y.double(), ga=ga.double(), v=v.double(), ua=ua.double())
    return dict(u=u, xdir=xdir, uy=uy, vsums=torch.cat([sv, svx, svgy]), rsums=torch.cat([suz, suzx, sxd, sxdx]),
                dgamma_vchain=svgy / gamma, dgamma_rev=suzx, dbeta_rev=suz, gy=gy, s1=torch.cat([s1a, s1b])), rounded


def ratios(got, ref, C):
    """error relative to the maximum of the reference, per output; every sum of a workspace against its own maximum"""
    out = {k: relmax(got[k], ref[k]) for k in ("gy",) + OUTPUT_KEYS + ("dgamma_vchain", "dgamma_rev", "dbeta_rev")}
    for k, names in (("s1", ("sum_gz", "sum_gz_xhat")), ("vsums", ("sum_v", "sum_v_xhat", "sum_v_gy")), ("rsums", ("sum_uz", "sum_uz_xhat", "sum_xdir", "sum_xdir_xhat"))):
        for i, nm in enumerate(names):
            out[nm] = relmax(got[k][i * C:(i + 1) * C], ref[k][i * C:(i + 1) * C])
    return out


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("shape", bn_ref.SHAPES)
def test_rounding_stays_within_half_the_tolerance(shape, storage):
    """fp32 arithmetic and storage-type rounding alone cost at most half of each tolerance of tests/test_bn2_gpu.py against the fp64
    closed form on the same rounded inputs, at every shape it runs: what a tolerance has to leave room for is rounding, not an error."""
    rows, C = shape
    tol = bn_ref.TOL[storage]
    worst = {}
    for kind in bn_ref.UA_KINDS:
        got, rounded = emulate(bn_ref.inputs(rows, C, seed=0, kind=kind), 0.2, storage == "bf16")
        ref = bn_ref.second_order(slope=0.2, **rounded)
        for k, r in ratios(got, ref, C).items():
            worst[k] = max(worst.get(k, 0.0), r)
    print(f"{shape} {storage}: " + ", ".join(f"{k} {r:.2e}" for k, r in worst.items()))
    for k, r in worst.items():
        limit = 0.5 * (tol["tensor"] if k in ("gy",) + OUTPUT_KEYS else tol["sums"])
        assert r <= limit, f"{shape} {storage}: {k} is off by {r:.3e} of its maximum > {limit:.1e}"
