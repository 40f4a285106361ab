"""fp64 restatement of one training-mode BatchNorm + LeakyReLU / ReLU layer on [rows, C] data and of its first and second backward,
for tests/test_bn2_math.py, tests/test_bn2_gpu.py and tests/test_bn_edges_gpu.py: plain torch, nothing shared with the code under test.

  xhat = (y - mean) / sigma, sigma = sqrt(biased var + eps), z = gamma * xhat + beta, a = z > 0 ? z : slope * z, s = act'(z)
  first backward:   gz = ga * s, m1 = mean gz, m2 = mean gz*xhat, gy = (gamma / sigma) (gz - m1 - xhat * m2)
  second backward of S = <v, gy> + <ua, a> (the notation above the bn2 kernels in csrc/bn2.hpp):
    xdir = -(gamma / sigma) (v * m2 + gz * mean(v xhat))
    u    = dS/dga = s (gamma / sigma) (v - mean v - xhat * mean(v xhat))
    q    = gamma * uz + xdir, uz = ua * s
    uy   = dS/dy  = (q - mean q - xhat * mean(q xhat)) / sigma - sum(v gy) xhat / (sigma n)
    dS/dgamma = sum(v gy) / gamma + sum uz*xhat,  dS/dbeta = sum uz
"""
import torch

EPS = 1e-5
# the terms second_order(drop=...) can leave out, and the output each of them belongs to
TERMS = {"xdir:v*m2": "xdir", "xdir:gz*mvx": "xdir", "u:mean_v": "u", "u:xhat*mvx": "u", "uy:mean_q": "uy", "uy:xhat*mqx": "uy",
         "uy:svgy": "uy"}
UA_KINDS = ("normal", "zero")
# what tests/test_bn2_gpu.py runs, and what tests/test_bn2_math.py therefore holds the inputs and the tolerances to.
# (rows, C): 8-channel units only / C < 64 / count 2 / several passes of the fused apply / exactly at the reduction's 256-workgroup cap,
# ragged / past the cap / maximum C / the 128-pixel topology's width
SHAPES = [(37, 8), (37, 32), (2, 64), (16384 + 37, 64), (16384 + 5, 128), (4096 + 37, 512), (1024 + 5, 2048), (37, 1024)]
# relative to the maximum of the reference; the first-order BatchNorm tests' (tests/test_ops_gpu.py: test_bn_act)
TOL = {"f32": {"tensor": 2e-5, "sums": 2e-5}, "bf16": {"tensor": 2e-2, "sums": 1e-2}}


def _stats(y):
    y = y.double()
    n = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    return mean, var, var * (n / max(n - 1, 1))


def first_order(y, ga, gamma, beta, slope):
    y, ga, gamma, beta = y.double(), ga.double(), gamma.double(), beta.double()
    mean, var, unbiased = _stats(y)
    sigma = torch.sqrt(var + EPS)
    xhat = (y - mean) / sigma
    z = gamma * xhat + beta
    s = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    gz = ga * s
    sgz, sgzx = gz.sum(0), (gz * xhat).sum(0)
    n = y.shape[0]
    gy = gamma / sigma * (gz - sgz / n - xhat * (sgzx / n))
    return dict(a=z * s, gy=gy, sgz=sgz, sgzx=sgzx, dgamma=sgzx, dbeta=sgz, mean=mean, var=var, unbiased=unbiased,
                xhat=xhat, sigma=sigma, s=s, gz=gz, z=z)


def second_order(y, ga, v, ua, gamma, beta, slope, drop=None):
    assert drop is None or drop in TERMS, drop
    keep = lambda name: 0.0 if drop == name else 1.0
    f = first_order(y, ga, gamma, beta, slope)
    v, ua, gamma = v.double(), ua.double(), gamma.double()
    xhat, sigma, s, gz, gy = f["xhat"], f["sigma"], f["s"], f["gz"], f["gy"]
    n = y.shape[0]
    gs = gamma / sigma
    m2 = f["sgzx"] / n
    sv, svx, svgy = v.sum(0), (v * xhat).sum(0), (v * gy).sum(0)
    xdir = -gs * (keep("xdir:v*m2") * v * m2 + keep("xdir:gz*mvx") * gz * (svx / n))
    u = s * gs * (v - keep("u:mean_v") * sv / n - keep("u:xhat*mvx") * xhat * (svx / n))
    uz = ua * s
    suz, suzx, sxd, sxdx = uz.sum(0), (uz * xhat).sum(0), xdir.sum(0), (xdir * xhat).sum(0)
    q = gamma * uz + xdir
    uy = (q - keep("uy:mean_q") * q.mean(0) - keep("uy:xhat*mqx") * xhat * (q * xhat).mean(0)) / sigma \
        - keep("uy:svgy") * svgy * xhat / (sigma * n)
    return dict(u=u, xdir=xdir, uy=uy, vsums=torch.cat([sv, svx, svgy]), rsums=torch.cat([suz, suzx, sxd, sxdx]),
                dgamma_vchain=svgy / gamma, dgamma_rev=suzx, dbeta_rev=suz, gy=gy, s1=torch.cat([f["sgz"], f["sgzx"]]), first=f)


def inputs(rows, C, seed=0, kind="normal"):
    """fp64 inputs in which every term of the second backward is O(1): ga and v are correlated with xhat and carry a channel mean,
    v also carries a part along the first backward's direction (so sum v*gy is far from 0).  One channel has gamma = -0.7 and one
    gamma = 1/64.  kind: "normal" (ua ~ N(0,1)) or "zero" (ua = 0, which leaves the xdir / sum(v gy) terms of uy alone)."""
    assert kind in UA_KINDS, kind
    g = torch.Generator().manual_seed(1000 + seed)
    N = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    y = 1.5 * N(rows, C) + 0.3
    if rows == 2:
        # count 2: xhat = +-1 / sqrt(1 + eps / var), so gy, u and uy are what a cancellation leaves, proportional to eps / (var + eps),
        # and a relative error d of the variance reaches them as d * var / (var + eps) / (eps / (var + eps)) = d * var / eps.  The
        # statistics rows are fp32 sums, d = 2^-24 E[y^2] / var: 2^-24 E[y^2] / eps ~ 1e-2 of the output, whatever the kernels do.
        # On a 2^-7 grid sum y and sum y^2 are exact in fp32 (21 bits) and the case tests the kernels, not the fp32 rows.
        y = torch.round(y * 128) / 128
    mean, var, _ = _stats(y)
    xhat = (y - mean) / torch.sqrt(var + EPS)
    ga = 0.6 * xhat + 0.5 + N(rows, C)
    v = 0.5 * xhat + 1.0 + 0.7 * (ga - ga.mean(0) - xhat * (ga * xhat).mean(0)) + 0.5 * N(rows, C)
    ua = N(rows, C)
    if kind == "zero":
        ua = torch.zeros_like(ua)
    gamma = 1 + 0.1 * N(C)
    gamma[1], gamma[2] = -0.7, 1.0 / 64
    beta = 0.1 * N(C)
    return dict(y=y, ga=ga, v=v, ua=ua, gamma=gamma, beta=beta)
