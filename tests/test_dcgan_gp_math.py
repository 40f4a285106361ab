"""The DCGAN gradient penalty back-propagated (the opt-in JCK_ENGINE_GP_BACKWARD engines): a double
backward through conv, train-mode BatchNorm, LeakyReLU, the conv5 head (k4 s1 p0 on the 4x4 map: ONE dot product per image)
and the sigmoid.  This file holds the closed-form reverse pass the HIP path implements (csrc/engine.hip, family 0 with the
flag: the trunk sweeps of family 1 plus the head step of jck_gp_head2_conv) and checks it against
autograd(create_graph=True) in fp64 on a small net of the same structure.  CPU only."""
import torch
import torch.nn.functional as F

dt = torch.float64
eps, lam, slope = 1e-5, 10.0, 0.2


def _net(B, L=2, H=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    chans = [3] + [8 << i for i in range(L)]
    Ws = [torch.randn(chans[i + 1], chans[i], 4, 4, dtype=dt, generator=g) * 0.1 for i in range(L)]
    gam = [1 + 0.1 * torch.randn(chans[i + 1], dtype=dt, generator=g) for i in range(L)]
    bet = [0.1 * torch.randn(chans[i + 1], dtype=dt, generator=g) for i in range(L)]
    w5 = torch.randn(1, chans[-1], 4, 4, dtype=dt, generator=g) * 0.1
    x = torch.randn(B, 3, H, H, dtype=dt, generator=g)
    assert H >> L == 4, "conv5 reads a 4x4 map"
    return Ws, gam, bet, w5, x


def _autograd(Ws, gam, bet, w5, x):
    params = Ws + gam + bet + [w5]
    ps = [p.clone().requires_grad_(True) for p in params]
    L = len(Ws)
    xi = x.clone().requires_grad_(True)
    h = xi
    for i in range(L):
        h = F.conv2d(h, ps[i], None, 2, 1)
        h = F.batch_norm(h, None, None, ps[L + i], ps[2 * L + i], True, 0.1, eps)
        h = F.leaky_relu(h, slope)
    p = torch.sigmoid(F.conv2d(h, ps[-1], None, 1, 0))
    gx = torch.autograd.grad(p, xi, torch.ones_like(p), create_graph=True)[0]
    gp = ((gx.flatten(1).norm(2, dim=1) - 1) ** 2).mean()
    return gx.detach(), torch.autograd.grad(lam * gp, ps)


def _closed_form(Ws, gam, bet, w5, x):
    """The engine's arithmetic: trunk forward, first backward, v-chain, head step, reverse sweep."""
    L, B = len(Ws), x.shape[0]
    n = lambda t: t.shape[0] * t.shape[2] * t.shape[3]
    cm = lambda t: t.mean((0, 2, 3), keepdim=True)
    cs = lambda t: t.sum((0, 2, 3))
    G = {"W": [torch.zeros_like(w) for w in Ws], "gam": [torch.zeros_like(v) for v in gam],
         "bet": [torch.zeros_like(v) for v in bet], "w5": torch.zeros_like(w5)}
    a, xh, sig, s = [x], [], [], []
    for i in range(L):
        y = F.conv2d(a[-1], Ws[i], None, 2, 1)
        mu = cm(y); sg = torch.sqrt(cm((y - mu) ** 2) + eps); sig.append(sg)
        xhat = (y - mu) / sg; xh.append(xhat)
        z = gam[i].view(1, -1, 1, 1) * xhat + bet[i].view(1, -1, 1, 1)
        s.append(torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope)))
        a.append(torch.where(z > 0, z, slope * z))
    a4 = a[-1].flatten(1)                                  # [B, K]: the head's input, any fixed element order
    wv = w5.flatten()                                      # [K] in the same order
    p = torch.sigmoid(a4 @ wv)                             # l_n = <a4_n, w5>
    sn = p * (1 - p)
    # first backward: g_a4,n = s_n * w5
    ga = (sn[:, None] * wv[None, :]).view_as(a[-1])
    gz, gy, m2 = [None] * L, [None] * L, [None] * L
    for i in reversed(range(L)):
        gz[i] = ga * s[i]
        m1 = cm(gz[i]); m2[i] = cm(gz[i] * xh[i])
        gy[i] = gam[i].view(1, -1, 1, 1) / sig[i] * (gz[i] - m1 - xh[i] * m2[i])
        ga = F.conv_transpose2d(gy[i], Ws[i], None, 2, 1)
    gx = ga
    nrm = gx.flatten(1).norm(2, dim=1)
    u = (lam * 2.0 / B * (nrm - 1) / nrm).view(B, 1, 1, 1) * gx
    # v-chain (family 1's trunk loop, unchanged)
    xdir, sigexp = [None] * L, [None] * L
    ui = u
    for i in range(L):
        v = F.conv2d(ui, Ws[i], None, 2, 1)
        G["W"][i] += torch.nn.grad.conv2d_weight(ui, Ws[i].shape, gy[i], 2, 1)
        gs = gam[i].view(1, -1, 1, 1) / sig[i]
        G["gam"][i] += cs(v * gy[i]) / gam[i]
        mvx = cm(v * xh[i])
        xdir[i] = -gs * (v * m2[i] + gz[i] * mvx)
        sigexp[i] = -(cs(v * gy[i]).view(1, -1, 1, 1) / sig[i])
        ui = gs * (v - cm(v) - xh[i] * mvx) * s[i]
    v4 = ui.flatten(1)
    # ---- the DCGAN head step (jck_gp_head2_conv)
    rs = (v4 @ wv) * (1 - 2 * p) * sn                      # logit adjoint
    G["w5"] += ((sn[:, None] * v4) + (rs[:, None] * a4)).sum(0).view_as(w5)
    ua = (rs[:, None] * wv[None, :]).view_as(a[-1])        # g_a4,n = rs_n * w5: the reverse sweep's input
    # reverse sweep (family 1's, unchanged)
    for i in reversed(range(L)):
        uz = ua * s[i]
        G["gam"][i] += cs(uz * xh[i]); G["bet"][i] += cs(uz)
        q = gam[i].view(1, -1, 1, 1) * uz + xdir[i]
        uy = (q - cm(q) - xh[i] * cm(q * xh[i])) / sig[i] + sigexp[i] * xh[i] / n(q)
        G["W"][i] += torch.nn.grad.conv2d_weight(a[i], Ws[i].shape, uy, 2, 1)
        ua = F.conv_transpose2d(uy, Ws[i], None, 2, 1)
    return gx, G["W"] + G["gam"] + G["bet"] + [G["w5"]]


def _check(B, L=2, H=16, seed=0):
    net = _net(B, L, H, seed)
    gx_ref, ref = _autograd(*net)
    gx, got = _closed_form(*net)
    assert float((gx - gx_ref).abs().max()) < 1e-13
    names = [f"W{i}" for i in range(L)] + [f"gam{i}" for i in range(L)] + [f"bet{i}" for i in range(L)] + ["w5"]
    for nm, g, r in zip(names, got, ref):
        assert float((g - r).abs().max()) < 1e-12 * max(1.0, float(r.abs().max())), nm


def test_dcgan_double_backward_matches_autograd():
    _check(B=4)


def test_dcgan_double_backward_one_image_and_three_stages():
    _check(B=1, seed=1)
    _check(B=3, L=3, H=32, seed=2)


def test_head_step_alone():
    """The head step in isolation: for l = <a, w>, p = sigmoid(l), the adjoint of the first backward g_a = p(1-p) w along v gives
    the logit adjoint rs = <v, w>(1-2p)p(1-p), d w = p(1-p) v + rs a, d a = rs w."""
    g = torch.Generator().manual_seed(3)
    K = 32
    a = torch.randn(K, dtype=dt, generator=g).requires_grad_(True)
    w = torch.randn(K, dtype=dt, generator=g).requires_grad_(True)
    v = torch.randn(K, dtype=dt, generator=g)
    p = torch.sigmoid(a @ w)
    ga = torch.autograd.grad(p, a, create_graph=True)[0]
    da, dw = torch.autograd.grad(ga @ v, (a, w))
    with torch.no_grad():
        p_, sn = p.detach(), p.detach() * (1 - p.detach())
        rs = (v @ w) * (1 - 2 * p_) * sn
        assert float((dw - (sn * v + rs * a)).abs().max()) < 1e-14
        assert float((da - rs * w).abs().max()) < 1e-14
