"""The second-order BatchNorm kernels of the back-propagated gradient penalty (jck_bn2_vchain, jck_bn2_reverse) against the fp64
closed form of tests/bn_ref.py, which tests/test_bn2_math.py holds to fp64 autograd.

The chain runs as the engine runs it, on device-produced intermediates: jck_bn_finalize_grouped (statistics rows built in fp64 and
rounded once to fp32) -> jck_bn_act_bwd (gy, the first backward's sums) -> jck_bn2_vchain (u, xdir, {sum v, sum v*xhat, sum v*gy},
dgamma += sum v*gy / gamma) -> jck_bn2_reverse (uy, {sum uz, sum uz*xhat, sum xdir, sum xdir*xhat}, dgamma += sum uz*xhat,
dbeta += sum uz).  The reference sees only the storage-rounded y, ga, v, ua and computes gy and the sums itself.  Inputs:
bn_ref.inputs, in which leaving out any one term moves its output by >= 3x the bf16 tolerance (asserted in test_bn2_math.py), with
ua ~ N(0,1) and ua = 0.  Tolerances, relative to the maximum of the reference: bn_ref.TOL, the first-order BatchNorm tests' - fp32
storage 2e-5; bf16 2e-2 for tensors, 1e-2 for sums and parameter gradients; every sum of a workspace against ITS OWN maximum.

Measured worst error / maximum over all shapes, both launch forms and both ua (MI355X):
                          fp32 storage (tol)     bf16 storage (tol)
  gy                      2.3e-6  (2e-5)         2.6e-3  (2e-2)
  u                       4.2e-6  (2e-5)         2.7e-3  (2e-2)
  xdir                    2.8e-7  (2e-5)         3.7e-3  (2e-2)
  uy                      3.3e-6  (2e-5)         6.6e-3  (2e-2)
  sum g_z, sum g_z*xhat   2.4e-7  (2e-5)         3.7e-7  (1e-2)
  sum v, sum v*xhat       2.7e-7  (2e-5)         2.2e-7  (1e-2)
  sum v*gy                1.9e-6  (2e-5)         1.8e-3  (1e-2)
  sum uz, sum uz*xhat     2.1e-7  (2e-5)         1.7e-7  (1e-2)
  sum xdir, sum xdir*xhat 4.1e-7  (2e-5)         2.3e-3  (1e-2)
  dgamma (v-chain)        2.0e-6  (2e-5)         1.4e-3  (1e-2)
  dgamma, dbeta (reverse) 2.1e-7  (2e-5)         1.7e-7  (1e-2)
The fp32 figures above 1e-6 all belong to (2, 64), where the outputs are what a cancellation leaves (bn_ref.inputs); elsewhere fp32
stays below 5e-7 and prec 2 (bf16x3, fp32 storage) below 4e-7.  The bf16 figures are the rounding of gy, xdir, u and uy to bf16 where
the kernels store them (the CPU emulation of tests/test_bn2_math.py gives the same 2e-3 .. 7e-3).  With `mean v` removed from the fused
v-chain apply, or the sum(v gy) term from the three-launch reverse apply, these tests fail at errors of 0.3 .. 17 of the maximum.
"""
import pytest
import torch

import bn_ref

pytestmark = pytest.mark.gpu

STORAGE = {1: "f32", 0: "bf16", 2: "f32"}          # prec 2 (bf16x3) stores fp32 and takes the float instantiation
VSUMS = ("sum_v", "sum_v_xhat", "sum_v_gy")
RSUMS = ("sum_uz", "sum_uz_xhat", "sum_xdir", "sum_xdir_xhat")


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def storage_round(inp, prec):
    """y, ga, v, ua as the library stores them and the fp32 parameters (fp64 values of those numbers)"""
    st = (lambda t: t.float().bfloat16().double()) if STORAGE[prec] == "bf16" else (lambda t: t.float().double())
    return dict(inp, gamma=inp["gamma"].float().double(), beta=inp["beta"].float().double(), **{k: st(inp[k]) for k in ("y", "ga", "v", "ua")})


def dev(t, prec):
    return t.to(torch.bfloat16 if STORAGE[prec] == "bf16" else torch.float32).cuda().contiguous()


def run_chain(G, prec, inp, slope, fuse, alias_u=False, vchain_dgamma=True, rev_grads=(True, True)):
    """-> dict of CPU results; workspaces start as NaN (an unwritten partial row shows), parameter gradients as ones (+= shows)"""
    rows, c = inp["y"].shape
    y, ga, v, ua = (dev(inp[k], prec) for k in ("y", "ga", "v", "ua"))
    gamma, beta = inp["gamma"].float().cuda(), inp["beta"].float().cuda()
    stats = torch.stack([inp["y"].sum(0), (inp["y"] ** 2).sum(0)]).float().unsqueeze(0).cuda().contiguous()    # [1 slot][2][C]
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")
    ones = lambda: torch.ones(c, device="cuda")
    st = G.cur_stream()
    G.lib.jck_tune(b"bn_bwd_fuse", fuse)
    try:
        aux = nan(4 * c)
        G.lib.jck_bn_finalize_grouped(stats, 1, float(rows), gamma, beta, bn_ref.EPS, aux, None, c, 1, st)
        s1, gy = nan(G.lib.jck_bn_bwd_ws_floats(c)), torch.empty_like(y)
        dg0, db0 = ones(), ones()
        G.lib.jck_bn_act_bwd(prec, ga, y, aux, slope, s1, gy, dg0, db0, rows, c, st)
        ws1, ws2 = nan(G.lib.jck_bn2_ws_floats(c)), nan(G.lib.jck_bn2_ws_floats(c))
        u = v if alias_u else torch.empty_like(v)
        xdir, uy = torch.empty_like(v), torch.empty_like(v)
        dg1, dg2, db2 = ones(), ones(), ones()
        G.lib.jck_bn2_vchain(prec, v, y, gy, aux, s1, gamma, slope, ws1, u, xdir, dg1 if vchain_dgamma else None, rows, c, st)
        G.lib.jck_bn2_reverse(prec, ua, y, xdir, aux, gamma, ws1, slope, ws2, uy, dg2 if rev_grads[0] else None,
                              db2 if rev_grads[1] else None, rows, c, st)
        torch.cuda.synchronize()
    finally:
        G.lib.jck_tune(b"bn_bwd_fuse", 1)
    cpu = lambda t: t.double().cpu()
    return dict(u=cpu(u), xdir=cpu(xdir), uy=cpu(uy), gy=cpu(gy), s1=cpu(s1[:2 * c]), vsums=cpu(ws1[:3 * c]), rsums=cpu(ws2[:4 * c]),
                dgamma_vchain=cpu(dg1) - 1, dgamma_rev=cpu(dg2) - 1, dbeta_rev=cpu(db2) - 1, dgamma_first=cpu(dg0) - 1,
                dbeta_first=cpu(db0) - 1)


def compare(G, got, ref, prec, tag, skip=()):
    """every output against the reference; -> {output: error / maximum}"""
    tol = bn_ref.TOL[STORAGE[prec]]
    c = ref["dbeta_rev"].numel()
    ratio = {}
    for k in ("gy", "u", "xdir", "uy"):
        assert torch.isfinite(got[k]).all(), f"{tag}: {k} is not finite"
        ratio[k] = G.check(got[k], ref[k], tol["tensor"], f"{tag} {k}")
    ref = dict(ref, dgamma_first=ref["first"]["dgamma"], dbeta_first=ref["first"]["dbeta"])
    for k in ("dgamma_first", "dbeta_first", "dgamma_vchain", "dgamma_rev", "dbeta_rev"):
        if k not in skip:
            ratio[k] = G.check(got[k], ref[k], tol["sums"], f"{tag} {k}")
    for key, names in (("s1", ("sum_gz", "sum_gz_xhat")), ("vsums", VSUMS), ("rsums", RSUMS)):
        for i, nm in enumerate(names):
            ratio[nm] = G.check(got[key][i * c:(i + 1) * c], ref[key][i * c:(i + 1) * c], tol["sums"], f"{tag} {nm}")
    print(f"BN2 {tag}: " + " ".join(f"{k}={r:.2e}" for k, r in ratio.items()))
    return ratio


CASES = [(shape, prec, 0.2) for shape in bn_ref.SHAPES for prec in (1, 0)] + \
        [((4096 + 37, 512), 2, 0.2)] + [((16384 + 37, 64), prec, 0.0) for prec in (1, 0)]


@pytest.mark.parametrize("kind", bn_ref.UA_KINDS)
@pytest.mark.parametrize("shape,prec,slope", CASES)
def test_bn2_chain_vs_fp64(G, shape, prec, slope, kind):
    """Both launch forms (jck_tune bn_bwd_fuse 2: reduce + an apply that sums its own slice's partial rows, for either storage type;
    0: reduce, sums, apply; C < 64 takes the three launches whatever the setting) at the shapes of bn_ref.SHAPES."""
    rows, c = shape
    inp = storage_round(bn_ref.inputs(rows, c, seed=0, kind=kind), prec)
    ref = bn_ref.second_order(slope=slope, **inp)
    for fuse in (2, 0):
        got = run_chain(G, prec, inp, slope, fuse)
        compare(G, got, ref, prec, f"{rows}x{c} prec{prec} slope{slope} ua={kind} fuse{fuse}")


@pytest.mark.parametrize("fuse", [2, 0])
@pytest.mark.parametrize("prec", [1, 0])
def test_bn2_aliasing_and_optional_gradients(G, prec, fuse):
    """At (700, 64): u written over v (the header allows it); jck_bn2_vchain without dgamma; jck_bn2_reverse with only one of
    dgamma / dbeta, which writes neither (csrc/ops_bn.hip) - the outputs and the sums are what they are with everything passed."""
    rows, c = 700, 64
    inp = storage_round(bn_ref.inputs(rows, c, seed=7), prec)
    ref = bn_ref.second_order(slope=0.2, **inp)
    tag = f"700x64 prec{prec} fuse{fuse}"
    compare(G, run_chain(G, prec, inp, 0.2, fuse, alias_u=True), ref, prec, tag + " u=v")
    got = run_chain(G, prec, inp, 0.2, fuse, vchain_dgamma=False)
    compare(G, got, ref, prec, tag + " vchain dgamma=NULL", skip=("dgamma_vchain",))
    for rev_grads in ((True, False), (False, True)):
        got = run_chain(G, prec, inp, 0.2, fuse, rev_grads=rev_grads)
        compare(G, got, ref, prec, tag + f" reverse grads={rev_grads}", skip=("dgamma_rev", "dbeta_rev"))
        assert torch.equal(got["dgamma_rev"], torch.zeros(c, dtype=torch.float64)), "dgamma written although dbeta is NULL (or the reverse)"
        assert torch.equal(got["dbeta_rev"], torch.zeros(c, dtype=torch.float64)), "dbeta written although dgamma is NULL (or the reverse)"
