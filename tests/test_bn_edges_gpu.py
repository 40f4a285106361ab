"""First-order BatchNorm + activation kernels at edge statistics and at the capped backward geometry, against fp64 autograd of
F.batch_norm + LeakyReLU / ReLU on the CPU from the storage-rounded inputs.  Paths: jck_bn_finalize + jck_bn_act_fwd, jck_bn_fwd (one
launch, with its running-statistics and record outputs), jck_bn_act_bwd_grouped in both launch forms (jck_tune bn_bwd_fuse 2 / 0).
jck_bn_act_bwd_res is not run here: its launch geometry depends on the chip's CU count, and tests/test_bn_resident_gpu.py owns it.

Tolerances, relative to the maximum of the reference: those of test_bn_act / test_bn_bwd_two_launches in tests/test_ops_gpu.py - output
1e-5 (fp32 storage) / 1.5e-2 (bf16), g_y 2e-5 / 2e-2, dgamma / dbeta 2e-5 / 1e-2, mean, invstd and the running statistics 1e-5.
ga is correlated with xhat (bn_ref.inputs), so the mean-subtraction terms of the backward are O(1) of g_y.

test_bn_edge_statistics - dedicated channels of one (4101, 64) tensor, each ALSO compared on its own, against its own maximum (a wrong
value in a quiet channel must not hide under a loud one, and the constant channels, whose gamma / sigma is gamma / sqrt(eps), must not
set the scale of the others):
  CONST  every row 0.3 (not representable): reference variance exactly 0 -> invstd = 1 / sqrt(eps), output beta, unbiased variance 0
  CLAMP  a constant for which the variance the kernels form, sum y^2 / n - (sum y / n)^2 in double from the fp32 statistics rows,
         is NEGATIVE before the clamp (found by a search on the CPU and asserted): the `vard < 0 -> 0` branch
  ZERO   every row 0, beta = 0: z == 0 exactly; act'(0) = slope for LeakyReLU and 0 for ReLU, in torch and in the kernels
  MEAN8  mean = 8 standard deviations.  The statistics rows are rounded once from fp64: a relative error <= 2^-24 of sum y^2 is
         2^-24 E[y^2] = (1 + 64) 2^-24 var, one of sum y is 2 * 2^-24 mean^2 = 128 * 2^-24 var: together <= 193 * 2^-24 ~ 1.2e-5 of
         var, half of that, 6e-6, of invstd - inside the 1e-5 used here (derived, not tuned).
  NEG    gamma = -0.7;   SMALL  gamma = 1/64
The constant channels have gamma = 1/8 and beta = 1: the aux-table form a = scale * y + shift leaves an absolute error of about
2 ulp(|gamma c| / sqrt(eps)) ~ 4e-6 where xhat is 0, which is below 1e-5 of beta = 1 (and would not be of beta ~ 0.1).
A finding of this work, not asserted: where the pre-clamp variance of a constant channel comes out POSITIVE (0.3 at 4133 rows in fp32:
+4.1e-9), invstd is 2e-4 below 1 / sqrt(eps) - the rounding of the fp32 statistics rows, 2^-23 c^2, measured against eps; no kernel
can recover it.  The row count here, 4101, is one where 0.3 gives a variance <= 0 in both storage types (asserted).

Measured worst error / maximum (MI355X), fp32 | bf16 storage: edge statistics - output 8.3e-7 (the CLAMP channel; 1.4e-7 over the
channels with spread) | 3.3e-3, g_y 2.4e-7 | 3.5e-3, dgamma 3.3e-7 | 1.3e-6, dbeta 9.5e-8 | 1.1e-7, invstd 1.0e-7 | 1.3e-6 (MEAN8),
mean 6.2e-8 | 7.1e-8; capped geometry - output 2.3e-7 | 3.4e-3, g_y 2.3e-6 at count 2 and 3.0e-7 elsewhere | 3.1e-3,
dgamma / dbeta 2.0e-7 | 2.2e-7.

test_bn_capped_geometry - ordinary channels at count 2 and at the backward shapes with the reduction at / past its 256-workgroup cap,
where a thread owns more than four rows; test_bn_capped_geometry_grouped - groups = 3, grad_groups = 2 at (4096 + 37, 512).
"""
import pytest
import torch
import torch.nn.functional as F

import bn_ref

pytestmark = pytest.mark.gpu

EPS = bn_ref.EPS
TOL = {"f32": dict(a=1e-5, gy=2e-5, grad=2e-5, stat=1e-5), "bf16": dict(a=1.5e-2, gy=2e-2, grad=1e-2, stat=1e-5)}
STORAGE = {1: "f32", 0: "bf16"}
CONST, CLAMP, ZERO, MEAN8, NEG, SMALL = 5, 9, 12, 17, 1, 2          # NEG, SMALL: where bn_ref.inputs puts gamma = -0.7 and 1/64
DEDICATED = {"const": CONST, "clamp": CLAMP, "zero": ZERO, "mean8": MEAN8, "neg": NEG, "small": SMALL}
FLAT = (CONST, CLAMP, ZERO)                                          # channels without spread
CLAMP_CANDIDATES = (0.45, -0.9, 1.3, 0.85, 0.7, 1.1)


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def st_round(t, prec):
    return t.float().bfloat16().double() if STORAGE[prec] == "bf16" else t.float().double()


def dev(t, prec):
    return t.to(torch.bfloat16 if STORAGE[prec] == "bf16" else torch.float32).cuda().contiguous()


def kernel_variance(c, n):
    """the variance bn_finalize_kernel / bn_fwd_fused_kernel form for n rows of the constant c, BEFORE the clamp: double arithmetic on
    statistics rows that were rounded to fp32"""
    y = torch.full((n,), c, dtype=torch.float64)
    s, q = y.sum().float().double(), (y * y).sum().float().double()
    return float(q / n - (s / n) ** 2)


def autograd_ref(y, ga, gamma, beta, slope):
    """fp64 F.batch_norm (training) + activation and its backward; momentum 1 turns the running buffers into (mean, unbiased var)"""
    y, gm, bt = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    c = y.shape[1]
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    bn = F.batch_norm(y, rm, rv, gm, bt, True, 1.0, EPS)
    a = F.leaky_relu(bn, slope) if slope else F.relu(bn)
    a.backward(ga)
    var = y.detach().var(0, unbiased=False)
    return dict(a=a.detach(), gy=y.grad, dgamma=gm.grad, dbeta=bt.grad, mean=rm, unbiased=rv, invstd=1 / torch.sqrt(var + EPS))


def stats_rows(y, slots=1):
    """[slots][2][C] fp32 statistics rows: the rows dealt round-robin over the slots, each sum formed in fp64 and rounded once"""
    return torch.stack([torch.stack([y[k::slots].sum(0), (y[k::slots] ** 2).sum(0)]) for k in range(slots)]).float().cuda().contiguous()


def run_forward(G, prec, y, gamma, beta, slope, one_launch):
    rows, c = y.shape
    yd, gam, bet = dev(y, prec), gamma.float().cuda(), beta.float().cuda()
    stats = stats_rows(y)
    aux, a = torch.full((4 * c,), float("nan"), device="cuda"), torch.empty_like(yd)
    rm, rv, nbt = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    rec = torch.full((2 * c,), float("nan"), device="cuda")
    st = G.cur_stream()
    if one_launch:
        G.lib.jck_bn_fwd(prec, yd, stats, 1, float(rows), gam, bet, EPS, slope, a, aux, rec, rm, rv, nbt, 0.1, rows, c, 1, st)
    else:
        G.lib.jck_bn_finalize(stats, 1, float(rows), gam, bet, rm, rv, nbt, 0.1, EPS, aux, c, st)
        G.lib.jck_bn_act_fwd(prec, yd, aux, slope, a, rows, c, st)
    torch.cuda.synchronize()
    assert int(nbt) == 1
    cpu = lambda t: t.double().cpu()
    out = dict(a=cpu(a), mean=cpu(aux[2 * c:3 * c]), invstd=cpu(aux[3 * c:]), running_mean=cpu(rm), running_var=cpu(rv), aux=cpu(aux))
    if one_launch:
        out.update(rec_mean=cpu(rec[:c]), rec_unbiased=cpu(rec[c:]))
    return out


def run_backward(G, prec, y, ga, gamma, beta, slope, fuse, groups=1, grad_groups=1):
    """y, ga: [groups][rows][C] (or [rows][C]); aux from jck_bn_finalize_grouped; -> g_y, sums, dgamma, dbeta (started from ones)"""
    y3, ga3 = y.reshape(groups, -1, y.shape[-1]), ga.reshape(groups, -1, y.shape[-1])
    rows, c = y3.shape[1:]
    yd, gad, gam, bet = dev(y3, prec), dev(ga3, prec), gamma.float().cuda(), beta.float().cuda()
    stats = torch.cat([stats_rows(y3[k]) for k in range(groups)]).contiguous()
    aux = torch.full((groups, 4 * c), float("nan"), device="cuda")
    st = G.cur_stream()
    G.lib.jck_bn_finalize_grouped(stats, 1, float(rows), gam, bet, EPS, aux, None, c, groups, st)
    sums = torch.full((groups, G.lib.jck_bn_bwd_ws_floats(c)), float("nan"), device="cuda")
    gy, dg, db = torch.empty_like(yd), torch.ones(c, device="cuda"), torch.ones(c, device="cuda")
    G.lib.jck_tune(b"bn_bwd_fuse", fuse)
    try:
        G.lib.jck_bn_act_bwd_grouped(prec, gad, yd, aux, slope, sums, gy, dg, db, rows, c, groups, grad_groups, st)
        torch.cuda.synchronize()
    finally:
        G.lib.jck_tune(b"bn_bwd_fuse", 1)
    cpu = lambda t: t.double().cpu()
    return dict(gy=cpu(gy).reshape(y.shape), sums=cpu(sums[:, :2 * c]), dgamma=cpu(dg) - 1, dbeta=cpu(db) - 1)


def edge_inputs(prec, rows=4096 + 5, c=64):
    inp = bn_ref.inputs(rows, c, seed=11)
    y, gamma, beta = inp["y"], inp["gamma"], inp["beta"]
    y[:, CONST] = 0.3
    clamp_c = next((v for v in CLAMP_CANDIDATES if kernel_variance(float(st_round(torch.tensor(v), prec)), rows) < 0), None)
    assert clamp_c is not None, "no candidate constant reaches the clamp at this row count"
    y[:, CLAMP] = clamp_c
    y[:, ZERO] = 0.0
    y[:, MEAN8] = y[:, MEAN8] - 0.3 + 12.0                            # 1.5 N + 12
    gamma[CONST] = gamma[CLAMP] = 0.125
    beta[CONST] = beta[CLAMP] = 1.0
    beta[ZERO] = 0.0
    y = st_round(y, prec)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    xhat = (y - mean) / torch.sqrt(var + EPS)
    g = torch.Generator().manual_seed(77)
    ga = st_round(0.6 * xhat + 0.5 + torch.randn(rows, c, generator=g, dtype=torch.float64), prec)
    return y, ga, gamma.float().double(), beta.float().double(), clamp_c


def check_channels(G, got, ref, tol, what, dedicated=DEDICATED, flat=FLAT):
    """the channels with spread together (the dedicated ones among them included), then every dedicated channel against its own maximum"""
    c = ref.shape[-1]
    rest = [k for k in range(c) if k not in flat]
    r = {"all": G.check(got[..., rest], ref[..., rest], tol, what)}
    for name, k in dedicated.items():
        r[name] = G.check(got[..., k], ref[..., k], tol, f"{what}, channel {name}")
    return r


@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("prec", [1, 0])
def test_bn_edge_statistics(G, prec, slope):
    rows, c = 4096 + 5, 64
    y, ga, gamma, beta, clamp_c = edge_inputs(prec, rows, c)
    tol = TOL[STORAGE[prec]]
    # the cases are what they claim to be
    pre_clamp = kernel_variance(float(y[0, CLAMP]), rows)
    assert pre_clamp < 0, f"the clamp channel ({clamp_c}) no longer reaches the clamp: {pre_clamp:+.3e}"
    assert kernel_variance(float(y[0, CONST]), rows) <= 0, "the 0.3 channel's fp32 statistics rows give a positive variance at this row count"
    assert float(y[:, MEAN8].mean() / y[:, MEAN8].std()) > 7.5
    ref = autograd_ref(y, ga, gamma, beta, slope)
    for k in FLAT:
        assert float(ref["unbiased"][k]) <= 1e-25 and abs(float(ref["invstd"][k]) * EPS ** 0.5 - 1) < 1e-12
    assert torch.equal(ref["a"][:, ZERO], torch.zeros(rows, dtype=torch.float64))
    ratios = {}
    for one_launch in (False, True):
        got = run_forward(G, prec, y, gamma, beta, slope, one_launch)
        tag = "jck_bn_fwd" if one_launch else "jck_bn_finalize + jck_bn_act_fwd"
        ratios[tag + " a"] = check_channels(G, got["a"], ref["a"], tol["a"], tag + " output")
        ratios[tag + " mean"] = check_channels(G, got["mean"], ref["mean"], tol["stat"], tag + " mean")
        ratios[tag + " invstd"] = check_channels(G, got["invstd"], ref["invstd"], tol["stat"], tag + " invstd")
        rm, rv = 0.1 * ref["mean"], 0.9 + 0.1 * ref["unbiased"]
        G.check(got["running_mean"], rm, tol["stat"], tag + " running_mean")
        G.check(got["running_var"], rv, tol["stat"], tag + " running_var")
        for k in FLAT:                                              # variance exactly 0: clamped, not a small negative or positive number
            assert abs(float(got["invstd"][k]) * EPS ** 0.5 - 1) <= 1e-6, (tag, k, float(got["invstd"][k]))     # a few fp32 ulp; unclamped: 2e-4
        assert torch.equal(got["a"][:, ZERO], torch.zeros(rows, dtype=torch.float64)), tag + ": z == 0 must give 0"
        if one_launch:
            check_channels(G, got["rec_mean"], ref["mean"], tol["stat"], tag + " record mean")
            check_channels(G, got["rec_unbiased"], ref["unbiased"], tol["stat"], tag + " record variance",
                           dedicated={k: v for k, v in DEDICATED.items() if v not in FLAT})
            for k in FLAT:
                assert float(got["rec_unbiased"][k]) == 0.0, (tag, k, float(got["rec_unbiased"][k]))
    for fuse in (2, 0):
        got = run_backward(G, prec, y, ga, gamma, beta, slope, fuse)
        tag = f"jck_bn_act_bwd_grouped fuse{fuse}"
        ratios[tag + " gy"] = check_channels(G, got["gy"], ref["gy"], tol["gy"], tag + " g_y")
        ratios[tag + " dgamma"] = check_channels(G, got["dgamma"], ref["dgamma"], tol["grad"], tag + " dgamma")
        ratios[tag + " dbeta"] = check_channels(G, got["dbeta"], ref["dbeta"], tol["grad"], tag + " dbeta")
        G.check(got["sums"][0, :c], ref["dbeta"], tol["grad"], tag + " sum g_z")
        G.check(got["sums"][0, c:], ref["dgamma"], tol["grad"], tag + " sum g_z*xhat")
        if slope == 0.0:                                           # ReLU'(0) = 0: nothing flows through the all-zero channel
            assert not got["gy"][:, ZERO].any() and float(got["dbeta"][ZERO]) == 0.0
        else:                                                      # LeakyReLU'(0) = slope
            assert float(ref["dbeta"][ZERO]) != 0.0
    for k, r in ratios.items():
        print(f"BNEDGE prec{prec} slope{slope} {k}: " + " ".join(f"{n}={x:.2e}" for n, x in r.items()))


GEOMETRY = [(2, 64), (37, 8), (4096 + 37, 512), (16384 + 5, 128), (1024 + 5, 2048)]


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("shape", GEOMETRY)
def test_bn_capped_geometry(G, shape, prec):
    rows, c = shape
    inp = bn_ref.inputs(rows, c, seed=0)            # the data tests/test_bn2_math.py bounds the fp32 rounding of, g_y at count 2 included
    y, ga = st_round(inp["y"], prec), st_round(inp["ga"], prec)
    gamma, beta = inp["gamma"].float().double(), inp["beta"].float().double()
    tol = TOL[STORAGE[prec]]
    ref = autograd_ref(y, ga, gamma, beta, 0.2)
    quiet = {"neg": NEG, "small": SMALL}
    for one_launch in (False, True):
        got = run_forward(G, prec, y, gamma, beta, 0.2, one_launch)
        tag = f"{rows}x{c} " + ("jck_bn_fwd" if one_launch else "jck_bn_finalize + jck_bn_act_fwd")
        r = check_channels(G, got["a"], ref["a"], tol["a"], tag + " output", quiet, ())
        G.check(got["mean"], ref["mean"], tol["stat"], tag + " mean")
        G.check(got["invstd"], ref["invstd"], tol["stat"], tag + " invstd")
        G.check(got["running_mean"], 0.1 * ref["mean"], tol["stat"], tag + " running_mean")
        G.check(got["running_var"], 0.9 + 0.1 * ref["unbiased"], tol["stat"], tag + " running_var")
        print(f"BNGEOM prec{prec} {tag}: " + " ".join(f"{n}={x:.2e}" for n, x in r.items()))
    for fuse in (2, 0):
        got = run_backward(G, prec, y, ga, gamma, beta, 0.2, fuse)
        tag = f"{rows}x{c} jck_bn_act_bwd_grouped fuse{fuse}"
        # count 2: xhat = +-1 / sqrt(1 + eps / var) and g_y is what gz - m1 - xhat * m2 leaves of its operands, eps / (var + eps) of them
        # (1e-5 where var ~ 1), so one fp32 rounding of xhat^2 is (var + eps) / eps * 2^-23 of a channel's OWN maximum; the tensor's
        # maximum belongs to the channel with the smallest variance, where it is not: the comparison over all channels stays
        r = check_channels(G, got["gy"], ref["gy"], tol["gy"], tag + " g_y", quiet if rows > 2 else {}, ())
        rg = check_channels(G, got["dgamma"], ref["dgamma"], tol["grad"], tag + " dgamma", quiet, ())
        rb = check_channels(G, got["dbeta"], ref["dbeta"], tol["grad"], tag + " dbeta", quiet, ())
        print(f"BNGEOM prec{prec} {tag}: gy " + " ".join(f"{n}={x:.2e}" for n, x in r.items()) + f" dgamma={rg['all']:.2e} dbeta={rb['all']:.2e}")


@pytest.mark.parametrize("fuse", [2, 0])
@pytest.mark.parametrize("prec", [1, 0])
def test_bn_capped_geometry_grouped(G, prec, fuse):
    """three groups with statistics of their own, the parameter gradients summed over the first two only"""
    groups, gg, rows, c = 3, 2, 4096 + 37, 512
    parts = [bn_ref.inputs(rows, c, seed=20 + k) for k in range(groups)]
    y, ga = (st_round(torch.stack([p[key] for p in parts]), prec) for key in ("y", "ga"))
    gamma, beta = parts[0]["gamma"].float().double(), parts[0]["beta"].float().double()
    tol = TOL[STORAGE[prec]]
    got = run_backward(G, prec, y, ga, gamma, beta, 0.2, fuse, groups, gg)
    dg, db = torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    quiet = {"neg": NEG, "small": SMALL}
    for k in range(groups):
        ref = autograd_ref(y[k], ga[k], gamma, beta, 0.2)
        r = check_channels(G, got["gy"][k], ref["gy"], tol["gy"], f"group {k} g_y", quiet, ())
        G.check(got["sums"][k, :c], ref["dbeta"], tol["grad"], f"group {k} sum g_z")
        G.check(got["sums"][k, c:], ref["dgamma"], tol["grad"], f"group {k} sum g_z*xhat")
        print(f"BNGROUP prec{prec} fuse{fuse} group {k}: " + " ".join(f"{n}={x:.2e}" for n, x in r.items()))
        if k < gg:
            dg += ref["dgamma"]
            db += ref["dbeta"]
    check_channels(G, got["dgamma"], dg, tol["grad"], "dgamma over the first two groups", quiet, ())
    check_channels(G, got["dbeta"], db, tol["grad"], "dbeta over the first two groups", quiet, ())
