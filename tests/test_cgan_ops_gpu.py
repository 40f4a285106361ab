"""Per-op parity of CGAN's discriminator head kernels (model/CGAN.py: label embedding, concat, Linear(8392,256) with its NCHW/NHWC
column permutation, Dropout, Linear(256,1), the penalty's second-order head terms; hipgan/functional.py:_CganHead) through the C ABI,
against float64 torch on the CPU built from the operands the kernels read (rounded to bf16 where the library stores bf16).

Tolerances are relative to max|ref| (gpu_util.check), per check and precision in TOL below, each at most ~4x the maximum error
measured on the MI355X over the check's cases (noted beside it) and never looser than: fp32-stored outputs of the f32 path 1e-5,
fp32 outputs from bf16 operands (fp32 accumulation) 2e-5, bf16-stored outputs 8e-3 (one bf16 ulp of the largest value).  Copies
and packs are held bitwise.  Every output is filled with NaN before its launch and must be written everywhere; what a kernel must
not touch (other columns of the concat buffer, padding, rows past B, buffer tails) holds a sentinel and must keep it.  Accumulating
outputs start from non-zero values.  The fused forms the engine runs (cg_head_mid, gp_head_mid_ev) are held bitwise to these
separate launches by tests/test_cgan_gpu.py::test_head_middle_in_one_launch_is_bitwise_the_four."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PRECS = [1, 0]
BATCHES = [1, 5, 63, 64, 65, 106, 300, 768]
NI, NO, SLOPE = 100, 200, 0.2                     # label embedding Linear(100, 200) + LeakyReLU(0.2)
FEAT, K1, KPAD, N1, KS = 8192, 8392, 8448, 256, 12   # conv features, Linear(8392, 256) in, padded, out, split-K
SCALE = 1.0 / 0.75                                # nn.Dropout(0.25)
SENT = -3.25                                      # sentinel of memory a kernel must not touch

# check -> {prec: tolerance}; the comment: maximum measured on the MI355X over the check's cases, f32 | bf16
TOL = {
    "embed_pre": {1: 8e-7, 0: 8e-7},            # 1.8e-7 | 1.8e-7   (fp32 on both paths: W, b fp32, labels exact)
    "embed_act": {1: 7e-7, 0: 8e-3},            # 1.7e-7 | 3.4e-3
    "embed_dW": {1: 3e-6, 0: 2e-6},             # 7.4e-7 | 4.6e-7
    "embed_db": {1: 1e-6, 0: 1e-6},             # 2.3e-7 | 2.2e-7
    "lin_slabs": {1: 3.5e-6, 0: 1e-6},          # 8.3e-7 | 2.3e-7
    "lin_h": {1: 3.5e-6, 0: 8e-3},              # 8.3e-7 | 3.3e-3
    "lin_hd": {1: 3.5e-6, 0: 8e-3},             # 8.4e-7 | 3.2e-3
    "lin_dgrad": {1: 3.5e-6, 0: 8e-3},          # 8.5e-7 | 2.7e-3
    "lin_wgrad": {1: 5e-6, 0: 2e-6},            # 1.3e-6 | 4.8e-7
    "lin_wgrad_forms": {1: 5e-6, 0: 2e-6},      # 1.1e-6 | 4.3e-7   (Z row chunks against one)
    "dropout": {1: 3e-7, 0: 8e-3},              # 6.8e-8 | 2.4e-3
    "colsum": {1: 7e-7, 0: 2e-7},               # 1.6e-7 | 4.7e-8
    "sum_vec": {1: 4e-7},                       # 9.2e-8
    "head_prob": {1: 1e-6, 0: 1.2e-6},          # 2.3e-7 | 2.9e-7
    "head_ds": {1: 1e-5, 0: 2e-5},              # 3.0e-6 | 4.6e-6
    "head_loss": {1: 1e-5, 0: 2e-5},            # 9.0e-6 | 4.6e-6   (logf(1 - p) of a p near 1, target 0.05)
    "gp_u": {1: 4e-7, 0: 8e-3},                 # 1.0e-7 | 2.7e-3
    "gp_rs": {1: 8e-7, 0: 7e-7},                # 2.0e-7 | 1.6e-7
    "gp_dw2": {1: 4e-7, 0: 6e-7},               # 9.2e-8 | 1.3e-7
}
# the head end to end, relative L2 per tensor: f32 4e-6 (measured <= 8.5e-7); bf16 about 4x the maximum measured over B (noted),
# every intermediate (embedding, hidden layer, gradients) stored as bf16
E2E_BF16 = {"prob": 1.9e-2,                     # 4.5e-3
            "a4": 1.6e-2,                       # 3.8e-3
            "label_embedding.weight": 1.4e-2,   # 3.4e-3
            "label_embedding.bias": 1.4e-2,     # 3.4e-3
            "linear1.weight": 1.4e-2,           # 3.5e-3
            "linear1.bias": 1.4e-2,             # 3.5e-3
            "linear2.weight": 1.2e-2,           # 2.9e-3
            "linear2.bias": 8.5e-3}             # 2.1e-3


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _chk(G, got, ref, name, prec, what=""):
    tol = TOL[name][prec]
    err = G.check(got, ref, tol, f"{name}[prec {prec}]{what}")
    print(f"measured {name} prec={prec}{what}: {err:.3e} (tol {tol:.1e})")


def _sync_cpu(t):
    torch.cuda.synchronize()
    return t.cpu()


def _dev(G, x, prec):
    """CPU tensor -> device tensor of the library's element type (bf16 rounding to nearest even, as the kernels store)."""
    return x.to(G.DT[prec]).cuda().contiguous()


def _r(G, x, prec):
    """What the kernel reads of a CPU fp32 tensor stored in the library's element type, as float64."""
    return G.rnd(x.float(), prec).double()


def _to_ours(x):
    """Reference column order (NCHW flatten of [*,512,4,4] + the rest) -> ours (NHWC flatten + the rest)."""
    n = x.shape[0]
    return torch.cat([x[:, :FEAT].reshape(n, 512, 4, 4).permute(0, 2, 3, 1).reshape(n, FEAT), x[:, FEAT:]], 1)


def _to_ref(x):
    """Ours -> the reference column order (the inverse of _to_ours)."""
    n = x.shape[0]
    return torch.cat([x[:, :FEAT].reshape(n, 4, 4, 512).permute(0, 3, 1, 2).reshape(n, FEAT), x[:, FEAT:]], 1)


def _filled(shape, prec_dt, rows_valid, fill=float("nan")):
    """[rows_valid + 1, ...] device buffer: the first rows_valid rows `fill`, the row past them SENT."""
    t = torch.full((rows_valid + 1,) + tuple(shape), fill, dtype=prec_dt, device="cuda")
    t[rows_valid] = SENT
    return t


def _is_sent(t):
    return bool((t.float() == SENT).all())


# ---- 1. label embedding: e = LeakyReLU(Linear(100, 200)(labels.float())) into cbuf[:, 8192:8392], and its backward ----------

def _labels(B, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "onehot":                    # class 7: no row selects it (nnz = 0 in label_embed_bwd_kernel)
        cls = torch.randint(0, NI - 1, (B,), generator=g)
        cls = cls + (cls >= 7).long()
        return F.one_hot(cls, NI).to(torch.int64)
    if kind == "one_class":                 # every row selects class 3
        return F.one_hot(torch.full((B,), 3), NI).to(torch.int64)
    lab = (torch.rand(B, NI, generator=g) < 0.1).to(torch.int64)       # multi-hot: Linear(labels.float()) of any counts
    lab[torch.rand(B, NI, generator=g) < 0.01] = 2
    lab[:, 0] = 1                            # a column every row selects
    lab[:, 7] = 0                            # and one no row selects
    return lab


def _embed_case(B, kind, seed):
    g = torch.Generator().manual_seed(seed)
    lab = _labels(B, kind, seed)
    W = torch.randn(NO, NI, generator=g) * 0.3
    b = torch.randn(NO, generator=g) * 0.1
    ue = torch.randn(B, NO, generator=g)                                 # dL/de, stored in cbuf's label columns
    dW0, db0 = torch.randn(NO, NI, generator=g) * 0.5, torch.randn(NO, generator=g) * 0.5
    return lab, W, b, ue, dW0, db0


def _embed_run(G, prec, lab, W, b, ue, dW0, db0, period=0):
    """fwd + bwd (the `_tiled` forms when period > 0): cbuf, pre, dW, db as the kernels leave them, after the sentinel checks."""
    B = ue.shape[0]
    dt = G.DT[prec]
    cbuf = _filled((KPAD,), dt, B, SENT)
    cbuf[:B, FEAT:FEAT + NO] = float("nan")
    pre = torch.full((B * NO + 64,), float("nan"), device="cuda")
    pre[B * NO:] = SENT
    labd = lab.cuda().contiguous()
    if period:
        G.lib.jck_label_embed_fwd_tiled(prec, labd, W.cuda(), b.cuda(), SLOPE, B, NI, NO, cbuf, KPAD, FEAT, pre, period, G.cur_stream())
    else:
        G.lib.jck_label_embed_fwd(prec, labd, W.cuda(), b.cuda(), SLOPE, B, NI, NO, cbuf, KPAD, FEAT, pre, G.cur_stream())
    torch.cuda.synchronize()
    c = cbuf.float().cpu()
    assert torch.isfinite(c[:B, FEAT:FEAT + NO]).all(), "label_embed_fwd left label columns unwritten"
    assert _is_sent(c[:, :FEAT]) and _is_sent(c[:, FEAT + NO:]) and _is_sent(c[B]), "label_embed_fwd wrote outside its columns"
    assert torch.isfinite(pre[:B * NO]).all() and _is_sent(pre[B * NO:]), "pre: unwritten or written past B rows"
    # backward: the gradient sits in the same columns of a [B][8448] buffer whose other columns are NaN (must not be read)
    gc = torch.full((B, KPAD), float("nan"))
    gc[:, FEAT:FEAT + NO] = ue
    gcd = _dev(G, gc, prec)
    dW = torch.cat([dW0.reshape(-1), torch.full((64,), SENT)]).cuda()
    db = torch.cat([db0, torch.full((64,), SENT)]).cuda()
    if period:
        G.lib.jck_label_embed_bwd_tiled(prec, gcd, KPAD, FEAT, pre, labd, SLOPE, B, NI, NO, dW, db, period, G.cur_stream())
    else:
        G.lib.jck_label_embed_bwd(prec, gcd, KPAD, FEAT, pre, labd, SLOPE, B, NI, NO, dW, db, G.cur_stream())
    torch.cuda.synchronize()
    dW, db = dW.cpu(), db.cpu()
    assert _is_sent(dW[NO * NI:]) and _is_sent(db[NO:]), "label_embed_bwd wrote past dW / db"
    return c, pre[:B * NO].cpu(), dW[:NO * NI].view(NO, NI), db[:NO]


def _embed_ref(G, prec, lab, W, b, ue):
    Wr, br = W.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.linear(lab.double(), Wr, br)
    e = F.leaky_relu(pre, SLOPE)
    e.backward(_r(G, ue, prec))
    return pre.detach(), e.detach(), Wr.grad, br.grad


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,kind", [(B, "onehot") for B in BATCHES] + [(5, "one_class"), (300, "one_class"), (5, "multihot"),
                                                                        (106, "multihot"), (768, "multihot")])
def test_label_embed(G, prec, B, kind):
    """jck_label_embed_fwd / _bwd against autograd of LeakyReLU(F.linear(labels.float(), W, b)): pre, the stored activation,
    dW and db (+=).  B > 256 and > 512 take two and three rounds of the ballot compaction in label_embed_bwd_kernel; a class
    column no row selects leaves its dW column bitwise as it was."""
    lab, W, b, ue, dW0, db0 = _embed_case(B, kind, 40 + B)
    c, pre, dW, db = _embed_run(G, prec, lab, W, b, ue, dW0, db0)
    pre_r, e_r, dW_r, db_r = _embed_ref(G, prec, lab, W, b, ue)
    _chk(G, pre.view(B, NO), pre_r, "embed_pre", prec)
    _chk(G, c[:B, FEAT:FEAT + NO], e_r, "embed_act", prec)
    _chk(G, dW.double() - dW0.double(), dW_r, "embed_dW", prec)
    _chk(G, db.double() - db0.double(), db_r, "embed_db", prec)
    unused = (lab != 0).sum(0) == 0
    assert bool(unused[7]) and torch.equal(dW[:, unused], dW0[:, unused]), "dW of an unselected class column changed"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("P,R", [(5, 2), (5, 3), (106, 2), (106, 3), (256, 2), (256, 3)])
def test_label_embed_tiled(G, prec, P, R):
    """`_tiled` with label_period = P over R*P rows (the engine's R2 / R3 rows of one batch's labels): bitwise the plain call on
    the explicitly repeated labels, and that against torch.  256 x 3 = 768 rows: three compaction rounds."""
    B = R * P
    lab, W, b, ue, dW0, db0 = _embed_case(P, "onehot", 70 + P)
    ue = torch.randn(B, NO, generator=torch.Generator().manual_seed(71 + B))
    tiled = _embed_run(G, prec, lab, W, b, ue, dW0, db0, period=P)
    plain = _embed_run(G, prec, lab.repeat(R, 1), W, b, ue, dW0, db0)
    for t, p, what in zip(tiled, plain, ("cbuf", "pre", "dW", "db")):
        assert torch.equal(t, p), f"_tiled {what} differs from the plain call on repeated labels"
    pre_r, e_r, dW_r, db_r = _embed_ref(G, prec, lab.repeat(R, 1), W, b, ue)
    _chk(G, plain[0][:B, FEAT:FEAT + NO], e_r, "embed_act", prec, " tiled")
    _chk(G, plain[2].double() - dW0.double(), dW_r, "embed_dW", prec, " tiled")
    _chk(G, plain[3].double() - db0.double(), db_r, "embed_db", prec, " tiled")


# ---- 2. concat / split of the conv features ------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", BATCHES)
def test_concat_split_rows(G, prec, B):
    """jck_concat_rows: cbuf[:, :8192] = a4 bitwise, the label columns / padding / row B keep their sentinel.  jck_split_rows: the
    reverse copy, nothing past B rows written."""
    g = torch.Generator().manual_seed(90 + B)
    dt = G.DT[prec]
    a4 = _dev(G, torch.randn(B, FEAT, generator=g), prec)
    cbuf = _filled((KPAD,), dt, B, SENT)
    G.lib.jck_concat_rows(prec, a4, FEAT, cbuf, KPAD, B, G.cur_stream())
    c = _sync_cpu(cbuf)
    assert torch.equal(c[:B, :FEAT], a4.cpu()), "concat_rows: feature columns differ from a4"
    assert _is_sent(c[:, FEAT:]) and _is_sent(c[B]), "concat_rows wrote outside [0, 8192) of the first B rows"
    gc = torch.randn(B, KPAD, generator=g)
    gc[:, FEAT:] = float("nan")
    gcd = _dev(G, gc, prec)
    ga4 = _filled((FEAT,), dt, B)
    G.lib.jck_split_rows(prec, gcd, KPAD, FEAT, ga4, B, G.cur_stream())
    s = _sync_cpu(ga4)
    assert torch.equal(s[:B], gcd[:, :FEAT].cpu()), "split_rows: copy differs"
    assert _is_sent(s[B]), "split_rows wrote past B rows"


# ---- 3. the Linear weight pack (NCHW -> NHWC columns) and its inverse for the gradient -----------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("N", [256, 250])
def test_pack_linear(G, prec, transpose, N):
    """jck_pack_linear(permC = 512, permHW = 16): the first 8192 columns reordered as torch's [N,512,4,4] -> [N,4,4,512], the label
    columns in place, padding rows and columns exactly zero; transpose = 1 is the [k'][n] dgrad operand."""
    g = torch.Generator().manual_seed(100 + N)
    w = torch.randn(N, K1, generator=g) * 0.05
    rows, cols = (N1, KPAD) if transpose == 0 else (KPAD, N1)
    wp = torch.full((rows * cols + 64,), float("nan"), dtype=G.DT[prec], device="cuda")
    wp[rows * cols:] = SENT
    G.lib.jck_pack_linear(prec, w.cuda(), N, K1, rows, cols, transpose, 512, 16, wp, G.cur_stream())
    got = _sync_cpu(wp)
    assert _is_sent(got[rows * cols:]), "pack_linear wrote past rows * cols"
    got = got[:rows * cols].view(rows, cols)
    exp = torch.zeros(N1, KPAD, dtype=G.DT[prec])
    exp[:N, :K1] = _to_ours(w).to(G.DT[prec])
    if transpose:
        exp = exp.t().contiguous()
    assert torch.equal(got, exp), f"pack_linear: {int((got != exp).sum())} elements differ (padding must be exactly 0)"


@pytest.mark.parametrize("N", [256, 250])
def test_unperm_linear_grad(G, N):
    """jck_unperm_linear_grad: grad[n][c*16+hw] (+)= gp[n][hw*512+c] (torch's [N,4,4,512] -> [N,512,4,4]), label columns in place,
    padding columns ignored; both accumulate modes, and the exact inverse of jck_pack_linear."""
    g = torch.Generator().manual_seed(110 + N)
    gp = torch.randn(N, KPAD, generator=g)
    gp[:, K1:] = float("nan")                                   # padding columns: never read
    exp = _to_ref(gp[:, :K1])

    def run(start, acc, src):
        grad = torch.cat([start.reshape(-1), torch.full((64,), SENT)]).cuda()
        G.lib.jck_unperm_linear_grad(src, N, K1, KPAD, 512, 16, grad, acc, G.cur_stream())
        out = _sync_cpu(grad)
        assert _is_sent(out[N * K1:]), "unperm_linear_grad wrote past N * K"
        return out[:N * K1].view(N, K1)

    assert torch.equal(run(torch.full((N, K1), float("nan")), 0, gp.cuda()), exp), "unperm (overwrite) differs"
    start = torch.randn(N, K1, generator=g)
    assert torch.equal(run(start, 1, gp.cuda()), start + exp), "unperm (accumulate) differs"
    # a packed fp32 gradient comes back exactly
    w = torch.randn(N, K1, generator=g)
    wp = torch.empty(N1 * KPAD, device="cuda")
    G.lib.jck_pack_linear(1, w.cuda(), N, K1, N1, KPAD, 0, 512, 16, wp, G.cur_stream())
    assert torch.equal(run(torch.full((N, K1), float("nan")), 0, wp), w)
    assert torch.equal(run(start, 1, wp), start + w)


# ---- 4.-6. Linear(8392, 256): forward (split-K + finish), input gradient, weight gradient ---------------------------------

def _lin_case(G, B, prec, seed):
    """x [B][8392] in the reference column order (bf16-representable for prec 0), its device copy in ours padded to 8448 with
    zeros (what concat + embedding leave in cbuf), W [256][8392] and its packed forward operand."""
    g = torch.Generator().manual_seed(seed)
    x = G.rnd(torch.randn(B, K1, generator=g) * 0.5, prec)
    w = torch.randn(N1, K1, generator=g) * 0.02
    xp = torch.zeros(B, KPAD)
    xp[:, :K1] = _to_ours(x)
    wp = torch.empty(N1 * KPAD, dtype=G.DT[prec], device="cuda")
    G.lib.jck_pack_linear(prec, w.cuda(), N1, K1, N1, KPAD, 0, 512, 16, wp, G.cur_stream())
    return g, x, w, _dev(G, xp, prec), wp


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", BATCHES)
def test_linear_fwd_split_k_and_finish(G, prec, B):
    """jck_linear_fwd (12 fp32 split-K slabs) + jck_linear_finish: h = x W^T + b, hd = h * mask * 4/3 (nn.Dropout(0.25) with a real
    0/1 mask), and the h = NULL, hd = NULL and bias = NULL forms."""
    g, x, w, xd, wp = _lin_case(G, B, prec, 120 + B)
    slab = torch.full((KS * B * N1 + 64,), float("nan"), device="cuda")
    slab[KS * B * N1:] = SENT
    G.lib.jck_linear_fwd(prec, xd, wp, None, slab, B, KPAD, N1, N1, KS, G.cur_stream())
    s = _sync_cpu(slab)
    assert torch.isfinite(s[:KS * B * N1]).all() and _is_sent(s[KS * B * N1:]), "split-K slabs: unwritten or written past"
    prod = x.double() @ _r(G, w, prec).t()
    _chk(G, s[:KS * B * N1].view(KS, B, N1).double().sum(0), prod, "lin_slabs", prec)
    bias = torch.randn(N1, generator=g) * 0.1
    mask = (torch.rand(B, N1, generator=g) >= 0.25).float()
    dt = G.DT[prec]
    for form in ("both", "no_h", "no_hd", "no_bias"):
        h, hd = _filled((N1,), dt, B), _filled((N1,), dt, B)
        G.lib.jck_linear_finish(prec, slab, KS, None if form == "no_bias" else bias.cuda(), mask.cuda(), SCALE,
                                None if form == "no_h" else h, None if form == "no_hd" else hd, B, N1, G.cur_stream())
        torch.cuda.synchronize()
        h_r = prod + (0 if form == "no_bias" else bias.double())
        for buf, ref, name, off in ((h, h_r, "lin_h", form == "no_h"), (hd, h_r * mask.double() * SCALE, "lin_hd", form == "no_hd")):
            t = buf.float().cpu()
            assert _is_sent(t[B]), f"linear_finish ({form}) wrote past B rows"
            if off:
                assert torch.isnan(t[:B]).all(), f"linear_finish ({form}) wrote {name} although it was NULL"
            else:
                _chk(G, t[:B], ref, name, prec, f" {form}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", BATCHES)
def test_linear_input_gradient(G, prec, B):
    """jck_linear_fwd on the transposed pack (Kpad = 256, N = NStore = 8448, ksplit = 1): g_cbuf = g_h W in our column order;
    un-permuted, against g_h @ W in the reference's; padding columns 8392..8447 exactly zero."""
    g = torch.Generator().manual_seed(130 + B)
    w = torch.randn(N1, K1, generator=g) * 0.02
    gh = G.rnd(torch.randn(B, N1, generator=g), prec)
    wt = torch.empty(KPAD * N1, dtype=G.DT[prec], device="cuda")
    G.lib.jck_pack_linear(prec, w.cuda(), N1, K1, KPAD, N1, 1, 512, 16, wt, G.cur_stream())
    gc = _filled((KPAD,), G.DT[prec], B)
    G.lib.jck_linear_fwd(prec, _dev(G, gh, prec), wt, None, gc, B, N1, KPAD, KPAD, 1, G.cur_stream())
    c = _sync_cpu(gc).float()
    assert torch.isfinite(c[:B]).all() and _is_sent(c[B]), "input gradient: unwritten or written past B rows"
    assert float(c[:B, K1:].abs().max()) == 0.0, "input gradient: padding columns must be zero"
    _chk(G, _to_ref(c[:B, :K1]), gh.double() @ _r(G, w, prec), "lin_dgrad", prec)


def _wgrad(G, prec, gyd, ldgy, xd, B, start):
    nb = G.lib.jck_linear_wgrad_ws_bytes(B, KPAD, N1)
    ws = torch.full((nb // 4,), float("nan"), device="cuda")
    gradp = torch.cat([start.reshape(-1), torch.full((64,), SENT)]).cuda()
    G.lib.jck_linear_wgrad(prec, gyd, ldgy, xd, KPAD, ws, nb, gradp, 0 if torch.isnan(start).all() else 1, B, N1, G.cur_stream())
    out = _sync_cpu(gradp)
    assert _is_sent(out[N1 * KPAD:]), "linear_wgrad wrote past N * Kpad"
    return out[:N1 * KPAD].view(N1, KPAD), gradp


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,accumulate,ldgy", [(B, 0, N1) for B in BATCHES] + [(B, 1, N1) for B in (5, 106, 768)] + [(65, 1, 264)])
def test_linear_weight_gradient(G, prec, B, accumulate, ldgy):
    """jck_linear_wgrad (N = 256, Kpad = 8448; row chunks rounded up to 64, so ragged last chunks) then jck_unperm_linear_grad,
    against autograd of F.linear on NCHW-flattened features: gy^T @ x."""
    g, x, _, xd, _ = _lin_case(G, B, prec, 140 + B)
    gy = G.rnd(torch.randn(B, N1, generator=g), prec)
    gyp = torch.full((B, ldgy), 1e6)                            # columns past N: must not be read
    gyp[:, :N1] = gy
    W = torch.zeros(N1, K1, dtype=torch.float64, requires_grad=True)
    F.linear(x.double(), W).backward(gy.double())
    start = torch.randn(N1, KPAD, generator=g) if accumulate else torch.full((N1, KPAD), float("nan"))
    gp, gpd = _wgrad(G, prec, _dev(G, gyp, prec), ldgy, xd, B, start)
    assert torch.isfinite(gp).all(), "linear_wgrad left elements unwritten"
    base = start if accumulate else torch.zeros(N1, KPAD)
    assert torch.equal(gp[:, K1:], base[:, K1:]), "linear_wgrad: padding columns must get exactly 0"
    if accumulate:
        _chk(G, _to_ref(gp[:, :K1].double() - start[:, :K1].double()), W.grad, "lin_wgrad", prec, " accumulate")
    else:
        gw = torch.full((N1 * K1,), float("nan"), device="cuda")
        G.lib.jck_unperm_linear_grad(gpd, N1, K1, KPAD, 512, 16, gw, 0, G.cur_stream())
        _chk(G, _sync_cpu(gw).view(N1, K1), W.grad, "lin_wgrad", prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [63, 300, 768])
def test_linear_weight_gradient_forms(G, prec, B):
    """The weight-gradient forms jck_tune exposes: wgrad_ws 0 and wgrad_dma 0 (the Linear layer's plain-matrix operand runs on the
    register-staged kernel either way: the same bits), wgrad_wgs 1024 (split over Z = 2 / 6 row chunks at B = 300 / 768 instead of
    one: the same result within the fp32 tolerance)."""
    g, x, _, xd, _ = _lin_case(G, B, prec, 150 + B)
    gyd = _dev(G, torch.randn(B, N1, generator=g), prec)
    nan = torch.full((N1, KPAD), float("nan"))
    ref, _ = _wgrad(G, prec, gyd, N1, xd, B, nan)
    defaults = {"wgrad_ws": 1, "wgrad_dma": 1, "wgrad_wgs": 256}
    for key, val in (("wgrad_ws", 0), ("wgrad_dma", 0), ("wgrad_wgs", 1024)):
        G.lib.jck_tune(key.encode(), val)
        try:
            got, _ = _wgrad(G, prec, gyd, N1, xd, B, nan)
        finally:
            G.lib.jck_tune(key.encode(), defaults[key])
        if key == "wgrad_wgs":
            _chk(G, got, ref, "lin_wgrad_forms", prec, f" {key}={val}")
        else:
            assert torch.equal(got, ref), f"{key}={val}: the weight gradient differs"


# ---- 7. dropout, bias-gradient sums --------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 1003, 106 * N1, 768 * N1])
def test_dropout(G, prec, n):
    """jck_dropout: y = x * mask * 4/3 with a 0/1 mask (forward and backward of nn.Dropout(0.25))."""
    g = torch.Generator().manual_seed(160 + n)
    x = G.rnd(torch.randn(n, generator=g), prec)
    mask = (torch.rand(n, generator=g) >= 0.25).float()
    y = torch.full((n + 64,), float("nan"), dtype=G.DT[prec], device="cuda")
    y[n:] = SENT
    G.lib.jck_dropout(prec, _dev(G, x, prec), mask.cuda(), SCALE, y, n, G.cur_stream())
    t = _sync_cpu(y).float()
    assert _is_sent(t[n:]), "dropout wrote past n"
    _chk(G, t[:n], x.double() * mask.double() * SCALE, "dropout", prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [1, 15, 16, 17, 49, 64, 65, 768])
def test_colsum(G, prec, B):
    """jck_colsum: db[j] += sum_b g[b][j] over N = 250 columns (not a multiple of 16) of rows ld = 264 apart; B reaches the 4-row
    unrolled loop and the tail loop.  Columns past N are not read, db past N not written."""
    N, ld = 250, 264
    g = torch.Generator().manual_seed(170 + B)
    x = G.rnd(torch.randn(B, N, generator=g), prec)
    xp = torch.full((B, ld), 1e6)
    xp[:, :N] = x
    db0 = torch.randn(N, generator=g)
    db = torch.cat([db0, torch.full((16,), SENT)]).cuda()
    G.lib.jck_colsum(prec, _dev(G, xp, prec), B, N, ld, db, G.cur_stream())
    t = _sync_cpu(db)
    assert _is_sent(t[N:]), "colsum wrote past N"
    _chk(G, t[:N].double() - db0.double(), x.double().sum(0), "colsum", prec)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_sum_vec(G, n):
    """jck_sum_vec: out[0] += sum_i x[i] (linear2's bias gradient); out[1] untouched."""
    g = torch.Generator().manual_seed(180 + n)
    x = torch.rand(n, generator=g) + 0.5
    out = torch.tensor([0.75, SENT]).cuda()
    G.lib.jck_sum_vec(x.cuda(), n, out, G.cur_stream())
    t = _sync_cpu(out)
    assert float(t[1]) == SENT
    _chk(G, t[:1].double() - 0.75, x.double().sum().view(1), "sum_vec", 1)


# ---- 8. the grouped head: Linear(256,1) / conv5 + sigmoid + BCE per group --------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("K,bias", [(N1, True), (FEAT, False)])
@pytest.mark.parametrize("G_,B", [(1, 37), (2, 37), (3, 37), (4, 37), (4, 1), (3, 255)])
def test_head_fwd_grouped(G, prec, K, bias, G_, B):
    """jck_head_fwd_grouped: G groups of B rows, each with its own target, mode and scalar slots.  Mode 0: ds = d mean-BCE / d logit
    as ATen's BCE (log clamped at -100, p(1-p) floored at 1e-12) per group; mode 1: ds = p(1-p).  The scalar table is indexed by the
    row inside its group; slots < 0 are not written."""
    g = torch.Generator().manual_seed(190 + 7 * G_ + B)
    targets, modes = [0.9, 0.0, 0.05, 1.0][:G_], [0, 1, 0, 0][:G_]
    slot_loss = [k if modes[k] == 0 else -1 for k in range(G_)]
    slot_p = [4 + k if k != 3 else -1 for k in range(G_)]
    a = G.rnd(torch.randn(G_ * B, K, generator=g), prec)
    w = torch.randn(K, generator=g) * (2.0 / K ** 0.5)
    b = torch.randn(1, generator=g) if bias else None
    prob = torch.full((G_ * B + 8,), float("nan"), device="cuda")
    ds = torch.full((G_ * B + 8,), float("nan"), device="cuda")
    prob[G_ * B:], ds[G_ * B:] = SENT, SENT
    ld = B + 3
    scal = torch.full((8, ld), SENT, device="cuda")
    i32 = lambda v: (ctypes.c_int * G_)(*v)                # the per-group table is read on the host
    G.lib.jck_head_fwd_grouped(prec, _dev(G, a, prec), w.cuda(), b.cuda() if bias else None, B, K, G_, (ctypes.c_float * G_)(*targets),
                               i32(modes), prob, ds, scal, i32(slot_loss), i32(slot_p), ld, G.cur_stream())
    torch.cuda.synchronize()
    prob, ds, scal = prob.cpu(), ds.cpu(), scal.cpu()
    assert _is_sent(prob[G_ * B:]) and _is_sent(ds[G_ * B:]), "head_fwd wrote past G*B rows"
    written = torch.zeros(8, ld, dtype=torch.bool)
    for k in range(G_):
        rows = slice(k * B, (k + 1) * B)
        s = (a[rows].double() @ w.double() + (b.double() if bias else 0)).requires_grad_(True)
        p = torch.sigmoid(s)
        if modes[k] == 0:
            loss_n = F.binary_cross_entropy(p, torch.full_like(p, targets[k]), reduction="none")
            loss_n.mean().backward()
            ds_r = s.grad
            _chk(G, scal[slot_loss[k], :B], loss_n.detach(), "head_loss", prec, f" group {k}")
            written[slot_loss[k], :B] = True
        else:
            ds_r = (p * (1 - p)).detach()
        _chk(G, prob[rows], p.detach(), "head_prob", prec, f" group {k}")
        _chk(G, ds[rows], ds_r, "head_ds", prec, f" group {k} mode {modes[k]}")
        if slot_p[k] >= 0:
            _chk(G, scal[slot_p[k], :B], p.detach(), "head_prob", prec, f" group {k} scalar table")
            written[slot_p[k], :B] = True
    assert _is_sent(scal[~written]), "head_fwd wrote scalar-table entries it does not own"


# ---- 9. the penalty's head terms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [1, 5])
def test_gp_grad(G, prec, N):
    """jck_gp_grad: u = coef*(||g||-1)/||g|| * g per NHWC4 image (the 4th channel zero) against autograd of
    coef/2 * sum_n (||g_n|| - 1)^2; an image with norm 0 gives 0."""
    HW, coef = 64 * 64, 2 * 10.0 / 5
    g = torch.Generator().manual_seed(200 + N)
    gr = torch.zeros(N, HW, 4)
    gr[..., :3] = G.rnd(torch.randn(N, HW, 3, generator=g) * 0.02, prec)
    if N > 1:
        gr[2] = 0
    norms = gr.double().reshape(N, -1).norm(dim=1)
    x = gr.double().requires_grad_(True)
    (coef / 2 * ((torch.linalg.vector_norm(x.reshape(N, -1), dim=1) - 1) ** 2).sum()).backward()
    u = torch.full((N * HW * 4 + 64,), float("nan"), dtype=G.DT[prec], device="cuda")
    u[N * HW * 4:] = SENT
    G.lib.jck_gp_grad(prec, _dev(G, gr, prec), norms.float().cuda(), coef, N, HW, u, G.cur_stream())
    t = _sync_cpu(u).float()
    assert _is_sent(t[N * HW * 4:]), "gp_grad wrote past N images"
    t = t[:N * HW * 4].view(N, HW, 4)
    assert float(t[..., 3].abs().max()) == 0.0
    if N > 1:
        assert float(t[2].abs().max()) == 0.0, "an image with norm 0 must give u = 0"
    _chk(G, t, x.grad, "gp_u", prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [1, 5, 63, 300])
def test_gp_head2(G, prec, B):
    """jck_gp_head2: rs = <ughd,w2> (1-2p) p(1-p) and dw2 += sum_n p(1-p) ughd against a float64 autograd double backward of
    p = sigmoid(h.w2 + b2): with g_h = d sum(p) / dh (grad_outputs = 1) and L = <ughd, g_h>, rs = dL/dlogit and dw2 = dL/dw2 minus
    its part through the logit (h^T rs, which the engine forms from rs)."""
    K = N1
    g = torch.Generator().manual_seed(210 + B)
    ughd = G.rnd(torch.randn(B, K, generator=g), prec)
    w2 = torch.randn(K, generator=g) * 0.06
    prob = torch.rand(B, generator=g) * 0.9 + 0.05
    dw0 = torch.randn(K, generator=g) * 0.1
    h = torch.randn(B, K, generator=g, dtype=torch.float64).requires_grad_(True)
    w = w2.double().requires_grad_(True)
    b2 = torch.logit(prob.double()) - (h @ w).detach()              # so that sigmoid(logit) is the prob the kernel reads
    logit = h @ w + b2
    p = torch.sigmoid(logit)
    g_h, = torch.autograd.grad(p, h, torch.ones_like(p), create_graph=True)
    rs_r, dw_r = torch.autograd.grad((g_h * ughd.double()).sum(), [logit, w])
    dw_r = dw_r - h.detach().t() @ rs_r
    rs = torch.full((B + 8,), float("nan"), device="cuda")
    rs[B:] = SENT
    dw2 = torch.cat([dw0, torch.full((8,), SENT)]).cuda()
    ws = torch.full((B + G.lib.jck_head_bwd_ws_floats(K),), float("nan"), device="cuda")
    G.lib.jck_gp_head2(prec, _dev(G, ughd, prec), w2.cuda(), prob.cuda(), B, K, rs, dw2, ws, G.cur_stream())
    torch.cuda.synchronize()
    rs, dw2 = rs.cpu(), dw2.cpu()
    assert _is_sent(rs[B:]) and _is_sent(dw2[K:]), "gp_head2 wrote past B / K"
    _chk(G, rs[:B], rs_r, "gp_rs", prec)
    _chk(G, dw2[:K].double() - dw0.double(), dw_r, "gp_dw2", prec)


# ---- 10. G's input [z | one-hot] ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [1, 5, 256])
def test_cgan_z(G, prec, B):
    """jck_cgan_z: [z | labels.float()] zero-padded to CiPad = 256 columns (model/CGAN.py:154-155), bitwise."""
    g = torch.Generator().manual_seed(220 + B)
    z = torch.randn(B, 100, generator=g)
    lab = F.one_hot(torch.randint(0, 100, (B,), generator=g), 100).to(torch.int64)
    out = _filled((256,), G.DT[prec], B)
    G.lib.jck_cgan_z(prec, z.cuda(), lab.cuda(), B, 100, 100, 256, out, G.cur_stream())
    t = _sync_cpu(out)
    exp = torch.cat([z, lab.float(), torch.zeros(B, 56)], 1).to(G.DT[prec])
    assert torch.equal(t[:B], exp), "cgan_z differs"
    assert _is_sent(t[B]), "cgan_z wrote past B rows"


# ---- 11. the head end to end: _CganHead's launch sequence ------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [1, 5, 37, 300])
def test_cgan_head_end_to_end(G, prec, B):
    """hipgan.functional._CganHead (concat, label embedding, pack, split-K Linear, finish + Dropout, head; backward: head, sum,
    dropout, weight gradient + unpermute, colsum, transposed pack, input gradient, split, embedding backward) against float64
    autograd of model/CGAN.py's head on NCHW features: probability, and the gradients of a4 and the six parameters, each in
    relative L2 (f32 4e-6; bf16 within E2E_BF16, measured with every intermediate stored as bf16)."""
    from hipgan.functional import _CganHead
    g = torch.Generator().manual_seed(230 + B)
    a4 = G.rnd(torch.randn(B, 512, 4, 4, generator=g), prec)
    lab = F.one_hot(torch.randint(0, 10, (B,), generator=g), 100).to(torch.int64)
    mask = (torch.rand(B, N1, generator=g) >= 0.25).float()
    params = {"label_embedding.weight": torch.randn(NO, NI, generator=g) * 0.1, "label_embedding.bias": torch.randn(NO, generator=g) * 0.1,
              "linear1.weight": torch.randn(N1, K1, generator=g) * 0.02, "linear1.bias": torch.randn(N1, generator=g) * 0.1,
              "linear2.weight": torch.randn(1, N1, generator=g) * 0.1, "linear2.bias": torch.randn(1, generator=g) * 0.1}
    gp = torch.rand(B, 1, generator=g) + 0.5
    # the reference: model/CGAN.py:111-123 in float64 (linear1's weight as the kernels read it: bf16 on the fast path)
    ref = {k: (_r(G, v, prec) if k == "linear1.weight" else v.double()).requires_grad_(True) for k, v in params.items()}
    xr = a4.double().requires_grad_(True)
    e = F.leaky_relu(F.linear(lab.double(), ref["label_embedding.weight"], ref["label_embedding.bias"]), SLOPE)
    h = F.linear(torch.cat([xr.flatten(1), e], 1), ref["linear1.weight"], ref["linear1.bias"]) * mask.double() * SCALE
    p_r = torch.sigmoid(F.linear(h, ref["linear2.weight"], ref["linear2.bias"]))
    (p_r * gp.double()).sum().backward()
    # the HIP path
    dev = {k: v.cuda().requires_grad_(True) for k, v in params.items()}
    a4d = G.to_nhwc(a4, prec).requires_grad_(True)
    p = _CganHead.apply(a4d, lab.cuda(), mask.cuda(), *dev.values(), prec)
    (p * gp.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = {"prob": (p.detach(), p_r.detach()), "a4": (G.from_nhwc(a4d.grad), xr.grad)}
    got.update({k: (dev[k].grad, ref[k].grad) for k in params})
    bad = []
    for k, (x, r) in got.items():
        x = x.detach().double().cpu().view(r.shape)
        assert torch.isfinite(x).all(), k
        l2 = ((x - r).norm() / (r.norm() + 1e-30)).item()
        lim = 4e-6 if prec == 1 else E2E_BF16[k]
        print(f"measured e2e {k} prec={prec} B={B}: rel-l2 {l2:.3e} (limit {lim:.1e})")
        if not l2 <= lim:
            bad.append(f"{k}: rel-l2 {l2:.3e} > {lim:.1e}")
    assert not bad, "; ".join(bad)
