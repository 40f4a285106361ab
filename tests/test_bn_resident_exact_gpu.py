"""The resident one-launch BatchNorm(+activation) backward, bn_bwd_res_kernel<NCH, NG> (csrc/bnres.hpp, jck_bn_act_bwd_res), checked on
what it does with its sums: bit for bit on data with one right answer, element by element on real statistics with a correlated gradient,
on edge channels, on non-finite gradients, and on when it runs at all.  bf16 storage, the only one the kernel has.

Every launch is planned first: jck_bn_res_plan (the function the launcher itself calls) says which instantiation (nch, ng) a case gets
and how many workgroups (nb) the chip gives, and the row counts are derived from it, per_iter = nb / (C / 64) * 64 rows per chunk index.
Every tensor the kernel writes (g_y, sums, dgamma, dbeta) is a view into a larger allocation whose guard regions hold a NaN bit pattern
and are compared as integers afterwards; the sums view is exactly groups * jck_bn_bwd_ws_floats(C) floats.  After every resident launch
jck_grid_sync_error is 0.  The barrier is never made to time out.

(a) test_exact_integer_data - the kernel's contract is the formula in the header of bnres.hpp evaluated with the aux it is GIVEN:
      g_z = z > 0 ? g_a : slope g_a,  z = scale y + shift,  d = y - mean,  t1 = sum g_z,  s2 = sum g_z d,  t2 = s2 invstd,
      m1 = t1 / n,  k2 = invstd (t2 / n),  g_y = scale ((g_z - m1) - d k2)
    y integers in [-4, 4], mean an integer in [-1, 1], invstd 1/2 or 1/4, gamma in {1, -1, 2, 1/2}, beta a multiple of 1/4, g_a integers
    in [-3, 3] = round(0.6 d + 0.5 + N(0, 1)), slope 0 or 0.25, n a power of two.  Asserted on the CPU before any launch, per case:
    sum |g_z| and sum |g_z d| per channel (times 4 for slope 0.25) < 2^24, so every partial sum in any order is exact in fp32; each of t1,
    s2, t2, t2 / n, m1, k2, g_z - m1, d k2, their difference and the product with scale survives fp64 -> fp32 -> fp64 unchanged, so every
    legal fma contraction gives the same bits; >= 5 % of the elements have z == 0 exactly (act'(0) = slope, as in torch); the mean terms
    reach >= 0.3 of max |g_y|; >= 500 distinct bf16 outputs; dgamma / dbeta (started from 3 and -2) stay exact.  The bit budget of the
    last difference is 3 (|.| < 8) + 2 (slope 0.25) + 2 a (invstd = 2^-a) + log2 n <= 24: the invstd values that do not fit a case are
    left out of that case (invstd 1/2 only from n = 2^16 at slope 0.25 and from n = 2^18 at slope 0; with 2 bits for the magnitude
    the 2^18-row case was not exact), nothing is widened.  Asserted with torch.equal: g_y == the bf16
    round-to-nearest-even of the fp64 value; sums == (t1 | t2); dgamma, dbeta == start + the sums over the groups < grad_groups;
    jck_bn_act_bwd_grouped gives the same g_y bits and sums.  One case per instantiation of the launcher's switch plus the multi-pass
    combinations: nch in {1, 2, 4, 8, 16} x groups in {1, 2, 3}, rows the power of two in (nch / 2 * per_iter, nch * per_iter].
    test_every_instantiation_is_planned compares the (nch, ng) of that table with the 12 of the switch.

(b) test_ragged_rows_true_statistics - y, g_a (correlated with xhat), gamma, beta from bn_ref.inputs, rounded to bf16; aux = the fp64
    statistics of the rounded y, rounded to fp32; reference bn_ref.first_order in fp64, group by group.  Out of place, then in place (same
    bits).  Per element
        |got - ref| <= half a bf16 ulp of max(|got|, |ref|) + E,
        E = K 2^-24 |scale| (|g_z| + A1 + Y invstd^2 A2),   A1 = mean |g_z|,  Y = |y| + |mean|,  A2 = mean (|g_z| Y)   (per channel)
    E has the shape the three terms of the kernel's expression give it, |g_z| + |m1| + |d k2|, with m1, d and k2 replaced by the
    majorants a rounding analysis can actually bound them by: A1 >= |m1|, Y >= |d|, invstd^2 A2 >= |k2|.  (The error of m1 is that of a
    sum, proportional to sum |g_z| and not to |sum g_z|; the error of d = y - fl(mean) is 2^-24 |mean| however small d is.)
    Derivation of K, with u = 2^-24 and first-order terms (one more for the second order):
      L = 59 additions at most on the path of a term through the kernel's sums: 16 chunks of a thread, 3 shuffles, 8 waves, 16 rows of a
          row lane of the cross-workgroup sum (256 rows at most: 4 trips of 4), 16 row lanes;
      g_z: 1 (slope * g_a);   m1 = fl(t1 * fl(1 / n)): L + 2, relative to A1;   d: fl(mean) and the subtraction, 2, relative to Y;
      k2 = fl(invstd * fl(fl(s2 * invstd) * fl(1 / n))): the terms fl(g_z * d) carry 1 + 2 + 1, the sum L, fl(invstd) twice 2, fl(1 / n)
          1, three products 3: L + 10, relative to invstd^2 A2;   d * k2: 2 + (L + 10) + 1 = L + 13;
      the two subtractions 1 each, fl(scale) 1, the last product 1 - on everything to their left.
      coefficient of |g_z|: 1 + 4 = 5;  of A1: L + 2 + 4 = L + 6;  of Y invstd^2 A2: L + 13 + 3 = L + 16;   K = L + 17 = 76.
    Sums, per channel: |t1 - sum g_z| <= (min(n, L) + 1) u sum |g_z|;  |t2 - sum g_z xhat| <= (min(n, L) + 6) u invstd sum |g_z| Y
    (6 = the roundings of one term: slope, fl(mean), y - mean, the product, fl(invstd), the product with it);  dgamma, dbeta (started
    from 3 and -2): the sum of those bounds over the groups < grad_groups + 4 u (|start| + sum of the groups' sum |terms|).
    n * 2^-24 * sum |terms| is the bound of a sequential sum; min(n, L) is what the kernel's tree gives and is never larger.
    A property of the inputs asserted on the CPU: no element has |z| within 4 u (|y scale| + |shift|) of 0 - there the kernel's fp32 z
    could take the other branch of the activation - except where y == 0 and the fp32 shift is 0, which is z == 0 in both.
    Rows: 1, 3, 63, 64, 65, per_iter - 1, per_iter, per_iter + 1, 4 per_iter + 37 (3 groups: two passes), 8 per_iter + 5 (3 groups: three
    passes), 16 per_iter - 1 (2 groups: two passes); C = 64 for the largest, 512 and more for the smallest.

(c) test_edge_channels - one (4 per_iter + 37, 64) tensor, three groups, slope 0.2 and 0: the channels ZERO (y == 0, beta 0: z == 0
    exactly), NEG (gamma -0.7) and SMALL (gamma 1/64) of tests/test_bn_edges_gpu.py, and JUMP, where group 1 has y / 4 + 3: its mean is
    shifted by 3 and its invstd is 4 times that of groups 0 and 2, so coefficients taken from a neighbouring group miss by far more
    than any bound.  (b)'s criterion over everything, then over every dedicated channel on its own.

(d) test_non_finite_gradient - one NaN / one +inf in g_a at a single (row, channel) of group 1 of 3 of (c)'s tensor (two passes): that
    channel of that group is non-finite in g_y and in the sums, as in the three-launch form (NaN for NaN; inf - inf = NaN for inf);
    dgamma / dbeta of the channel are non-finite exactly when 1 < grad_groups; everything else equals the clean run bit for bit.

(e) test_plan_refusals_and_fallbacks - jck_bn_res_plan returns 0 for fp32 storage, C = 32, C = 96, rows > 16 per_iter, bn_res = 0, and
    bn_res = 1 with several groups under the 120 MB threshold; for each but bn_res = 0 (tests/test_bn_resident_gpu.py has it)
    jck_bn_act_bwd_res does what jck_bn_act_bwd_grouped does: the same bits, or for C = 96, which no BatchNorm kernel takes, the same
    refusal with nothing written.

Measured on an MI355X (nb = 256, per_iter = 16384 rows at C = 64), nothing tuned to it.  (a): all 15 cases equal bit for bit, both
forms; the inputs had z == 0 in 8.0 to 10.2 % of the elements, mean terms of 0.76 to 1.01 of max |g_y|, 1010 to 3157 distinct outputs.
Worst error / bound, (b) and (c); g_y is at most 0.999 in every case and in every dedicated channel - the half ulp of the bf16 store is
nearly all of its bound, and the fp64 reference rounded to bf16 measures 0.998 against itself - so E is what decides only near g_y = 0:
  rows (groups x rows x C)      plan     g_y    sum g_z  sum g_z xhat  dgamma   dbeta
  1        1 x 1 x 512          (1, 1)   0      0.46     0             0        0.20     (g_y, xhat == 0 exactly at one row)
  3        2 x 3 x 1024         (1, 2)   0.996  0        0.37          0.23     0        (slope 0, three terms: sum g_z exact)
  63       3 x 63 x 2048        (1, 3)   0.998  0.038    0.043         0.032    0.028
  64       1 x 64 x 512         (1, 1)   0.997  0.0098   0.045         0        0        (grad_groups 0)
  65       2 x 65 x 1024        (1, 2)   0.998  0.038    0.042         0.028    0.029
  p - 1    1 x 2047 x 512       (1, 1)   0.998  0.053    0.039         0.037    0.050
  p        3 x 4096 x 256       (1, 3)   0.998  0.045    0.038         0.029    0.030
  p + 1    2 x 4097 x 256       (2, 2)   0.998  0.042    0.043         0.040    0.040
  4p + 37  3 x 32805 x 128      (8, 2)   0.998  0.036    0.033         0.025    0.028
  8p + 5   3 x 131077 x 64      (16, 1)  0.999  0.043    0.035         0.024    0.022
  16p - 1  2 x 262143 x 64      (16, 1)  0.998  0.038    0.034         0.032    0.036
  edge, slope 0.2  3 x 65573 x 64  (8, 2)  0.998  0.039  0.041         0.029    0.022    zero 0.997 neg 0.998 small 0.998 jump 0.997
  edge, slope 0    3 x 65573 x 64  (8, 2)  0.999  0.037  0.036         0.025    0.027    zero 0 (all 0) neg 0.998 small 0.997 jump 0.997
"""
import ctypes
import functools

import pytest
import torch

import bn_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
L_SUM = 59              # additions on the longest path of the kernel's sums (derived above)
K_ELEM = L_SUM + 17     # roundings behind one element of g_y (derived above)
GUARD = 4096
PAT = {2: 0x7FC1, 4: 0x7FC00BAD}                 # NaN bit patterns (bf16, fp32)
IDT = {2: torch.int16, 4: torch.int32}
DG0, DB0 = 3.0, -2.0                             # where dgamma / dbeta start
SWITCH = {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (1, 2), (2, 2), (4, 2), (8, 2), (1, 3), (2, 3), (4, 3)}     # BNRES_CASE in csrc/ops_bn.hip
ZERO, NEG, SMALL, JUMP = 12, 1, 2, 20            # NEG, SMALL: where bn_ref.inputs puts gamma = -0.7 and 1/64
DEDICATED = {"zero": ZERO, "neg": NEG, "small": SMALL, "jump": JUMP}


@pytest.fixture(scope="module")
def G():
    import gpu_util
    gpu_util.lib.jck_tune(b"bn_res", 2)        # the resident form whenever it fits (the default leaves small multi-group passes to the three launches)
    yield gpu_util
    gpu_util.lib.jck_tune(b"bn_res", 1)
    for cached in (exact_case, ragged_case, edge_case, clean_run):       # the references are large: not kept for the rest of the session
        cached.cache_clear()


# ---------------------------------------------------------------------------------------------------------------------
# plan, guarded buffers, launch
# ---------------------------------------------------------------------------------------------------------------------
def plan(G, rows, c, groups, prec=0):
    """(nch, ng, nb) of jck_bn_act_bwd_res for these arguments, None where it takes the three-launch form"""
    nch, ng, nb = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    if not G.lib.jck_bn_res_plan(prec, rows, c, groups, ctypes.byref(nch), ctypes.byref(ng), ctypes.byref(nb)):
        return None
    return nch.value, ng.value, nb.value


def per_iter(G, c):
    p = plan(G, 1, c, 1)
    assert p is not None and p[0] == 1 and p[1] == 1 and p[2] % max(c // 64, 8) == 0, (c, p)
    return p[2] // (c // 64) * 64


class Guarded:
    """numel elements of dtype between two guard regions of a fixed NaN bit pattern; the payload starts as the same pattern"""

    def __init__(self, numel, dtype, init=None):
        self.n, self.esz = int(numel), torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.empty(self.n + 2 * GUARD, dtype=dtype, device="cuda")
        self.ints = self.buf.view(IDT[self.esz])
        self.ints.fill_(PAT[self.esz])
        self.t = self.buf[GUARD:GUARD + self.n]
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def check(self, what):
        for name, region in (("before", self.ints[:GUARD]), ("after", self.ints[GUARD + self.n:])):
            bad = torch.nonzero(region != PAT[self.esz])
            assert bad.numel() == 0, f"{what}: {bad.shape[0]} guard elements {name} the buffer overwritten, first at {int(bad[0])}"

    def untouched(self):
        return bool((self.ints[GUARD:GUARD + self.n] == PAT[self.esz]).all())


def sync_ws(G):
    return torch.zeros(G.lib.jck_grid_sync_bytes() // 4, dtype=torch.int32, device="cuda")


def launch(G, y, ga, aux, slope, grad_groups, expect=None, resident=True, inplace=False, grads=True, prec=0, raises=False):
    """y, ga: [groups][rows][C] CPU tensors of the storage type; aux [groups][4C] fp32.  expect: the (nch, ng) the resident launch must
    be planned with, None: it must be planned as a fallback.  -> the CPU copies of what was written"""
    groups, rows, c = y.shape
    what = f"{'resident' if resident else 'three-launch'} {groups} x {rows} x {c}"
    ws = sync_ws(G) if resident else None
    if resident:
        p = plan(G, rows, c, groups, prec)
        assert (p and p[:2]) == expect, f"{what}: planned as {p}, the case is meant for {expect}"
    wsf = G.lib.jck_bn_bwd_ws_floats(c)
    yd, auxd = y.cuda().contiguous(), aux.float().cuda().contiguous()
    gy = Guarded(ga.numel(), ga.dtype, ga if inplace else None)
    gad = gy.t if inplace else ga.cuda().contiguous()
    sums = Guarded(groups * wsf, torch.float32)
    dg = Guarded(c, torch.float32, torch.full((c,), DG0)) if grads else None
    db = Guarded(c, torch.float32, torch.full((c,), DB0)) if grads else None
    args = (prec, gad, yd, auxd, slope, sums.t, gy.t, dg.t if grads else None, db.t if grads else None, rows, c, groups, grad_groups)
    err = None
    try:
        if resident:
            G.lib.jck_bn_act_bwd_res(*args, ws, G.cur_stream())
        else:
            G.lib.jck_bn_act_bwd_grouped(*args, G.cur_stream())
    except Exception as e:          # the wrapper raises on a non-zero return
        if not raises:
            raise
        err = str(e)
    torch.cuda.synchronize()
    if resident:
        assert G.lib.jck_grid_sync_error(ws) == 0, f"{what}: a grid barrier timed out"
    for name, buf in (("g_y", gy), ("sums", sums), ("dgamma", dg), ("dbeta", db)):
        if buf is not None:
            buf.check(f"{what} {name}")
    if raises:
        assert err is not None, f"{what}: the call was expected to be refused"
        assert gy.untouched() and sums.untouched() and bool((dg.t == DG0).all()) and bool((db.t == DB0).all()), f"{what}: refused, yet written"
        return err.split(": ", 1)[-1]
    return dict(gy=gy.t.view(groups, rows, c).cpu(), sums=sums.t.view(groups, wsf)[:, :2 * c].cpu(),
                dgamma=dg.t.cpu() if grads else None, dbeta=db.t.cpu() if grads else None)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(IDT[a.element_size()]), b.contiguous().view(IDT[b.element_size()]))


def first_diff(got, ref):
    bad = torch.nonzero(got != ref)
    if not bad.numel():
        return "no difference"
    i = tuple(bad[0].tolist())
    return f"{bad.shape[0]} of {got.numel()} differ, first at {i}: got {float(got[i])!r} want {float(ref[i])!r}"


# ---------------------------------------------------------------------------------------------------------------------
# (a) exact data
# ---------------------------------------------------------------------------------------------------------------------
# (nch, groups, C, slope, grad_groups, dgamma / dbeta given): C rotates, grad_groups runs from 0 to groups, the gradients are null once
EXACT = [(1, 1, 64, 0.25, 1, True), (1, 2, 128, 0.0, 0, True), (1, 3, 256, 0.25, 3, True),
         (2, 1, 512, 0.0, 0, True), (2, 2, 1024, 0.25, 2, True), (2, 3, 2048, 0.0, 1, True),
         (4, 1, 64, 0.25, 1, True), (4, 2, 128, 0.0, 1, True), (4, 3, 256, 0.25, 2, True),
         (8, 1, 512, 0.0, 1, False), (8, 2, 1024, 0.25, 0, True), (8, 3, 2048, 0.0, 3, True),
         (16, 1, 64, 0.0, 0, True), (16, 2, 128, 0.25, 2, True), (16, 3, 256, 0.0, 2, True)]


def expected_ng(nch, groups):
    """the resident groups of the launcher's switch: as many of the groups as fit 16 chunks, three at most"""
    return max(g for g in (1, 2, 3) if g <= groups and (g == 1 or g * nch <= 16))


def tier_rows(G, nch, c):
    """the power of two in (nch / 2 * per_iter, nch * per_iter], None if the chip leaves none"""
    top = nch * per_iter(G, c)
    rows = 1 << (top.bit_length() - 1)
    return rows if rows * 2 > top and plan(G, rows, c, 1)[0] == nch else None


def f32_exact(x):
    return torch.equal(x.float().double(), x)


@functools.lru_cache(maxsize=1)
def exact_case(rows, c, groups, slope, grad_groups):
    n, b = rows, rows.bit_length() - 1
    assert n == 1 << b
    gbits = 2 if slope else 0
    shifts = [a for a in (1, 2) if 3 + gbits + 2 * a + b <= 24]         # invstd = 2^-a that the bit budget of the last difference admits
    assert shifts, f"no invstd fits {n} rows at slope {slope}"
    mult = 4 if slope else 1
    g = torch.Generator().manual_seed(17 * b + c + groups)
    gamma = torch.tensor([1.0, -1.0, 2.0, 0.5], dtype=torch.float64)[torch.randint(0, 4, (c,), generator=g)]
    beta = torch.randint(-4, 5, (c,), generator=g).double() / 4
    y = torch.empty(groups, rows, c, dtype=torch.bfloat16)
    ga, gy = torch.empty_like(y), torch.empty_like(y)
    aux, sums = torch.empty(groups, 4 * c), torch.empty(groups, 2 * c)
    dg, db = torch.full((c,), DG0, dtype=torch.float64), torch.full((c,), DB0, dtype=torch.float64)
    dg_abs, db_abs = dg.abs(), db.abs()
    zeros, mean_part, out_max = 0, 0.0, 0.0
    hist = torch.zeros(65536, dtype=torch.int64)
    for k in range(groups):
        mean = torch.randint(-1, 2, (c,), generator=g).double()
        invstd = 0.5 ** torch.tensor(shifts, dtype=torch.float64)[torch.randint(0, len(shifts), (c,), generator=g)]
        scale = gamma * invstd
        shift = beta - mean * scale
        yk = (1.5 * torch.randn(rows, c, generator=g) + 0.3).round_().clamp_(-4, 4).double()
        d = yk - mean
        gak = (0.6 * d + 0.5 + torch.randn(rows, c, generator=g)).round_().clamp_(-3, 3)
        z = yk * scale + shift
        zeros += int((z == 0).sum())
        gz = torch.where(z > 0, gak, slope * gak)
        del z
        gd = gz * d
        assert float(gz.abs().sum(0).max()) * mult < 2 ** 24 and float(gd.abs().sum(0).max()) * mult < 2 ** 24, "partial sums leave fp32"
        t1, s2 = gz.sum(0), gd.sum(0)
        del gd
        t2 = s2 * invstd
        t2n, m1 = t2 / n, t1 / n
        k2 = invstd * t2n
        e1, e2 = gz - m1, d * k2
        e3 = e1 - e2
        out = scale * e3
        for name, v in (("t1", t1), ("s2", s2), ("t2", t2), ("t2 / n", t2n), ("m1", m1), ("k2", k2), ("g_z - m1", e1), ("d k2", e2),
                        ("the difference", e3), ("the product", out), ("aux", torch.cat([scale, shift]))):
            assert f32_exact(v), f"{name} is not exact in fp32 (group {k})"
        del e1, e2, e3
        mean_part = max(mean_part, float((out - scale * gz).abs().max()))
        out_max = max(out_max, float(out.abs().max()))
        y[k], ga[k], gy[k] = yk.bfloat16(), gak.bfloat16(), out.bfloat16()
        assert torch.equal(y[k].double(), yk) and torch.equal(ga[k].double(), gak)
        hist += torch.bincount(gy[k].view(torch.int16).reshape(-1).long() + 32768, minlength=65536)
        aux[k] = torch.cat([scale, shift, mean, invstd]).float()
        sums[k] = torch.cat([t1, t2]).float()
        if k < grad_groups:
            dg, db, dg_abs, db_abs = dg + t2, db + t1, dg_abs + t2.abs(), db_abs + t1.abs()
    assert float(max(dg_abs.max(), db_abs.max())) * mult * 4 < 2 ** 24, "dgamma / dbeta leave fp32"         # t2: multiples of 1 / (4 mult)
    assert zeros >= 0.05 * y.numel(), f"z == 0 in only {zeros / y.numel():.3f} of the elements"
    assert mean_part >= 0.3 * out_max, f"the mean terms reach only {mean_part / out_max:.2f} of max |g_y|"
    distinct = int((hist > 0).sum())
    assert distinct >= 500, f"only {distinct} distinct outputs"
    info = f"z==0 {zeros / y.numel():.3f} mean-part {mean_part / out_max:.2f} distinct {distinct} invstd 2^-{shifts}"
    return dict(y=y, ga=ga, aux=aux, gy=gy, sums=sums, dgamma=dg.float(), dbeta=db.float(), info=info)


@pytest.mark.parametrize("case", EXACT, ids=lambda t: f"nch{t[0]}-g{t[1]}-c{t[2]}")
def test_exact_integer_data(G, case):
    nch, groups, c, slope, gg, grads = case
    rows = tier_rows(G, nch, c)
    if rows is None:
        pytest.skip(f"this chip's workgroup count leaves no power of two in the {nch}-chunk tier at C = {c}")
    want = (nch, expected_ng(nch, groups))
    ref = exact_case(rows, c, groups, slope, gg)
    print(f"BNRESX exact {rows}x{c} groups {groups} plan {want}: {ref['info']}")
    got = launch(G, ref["y"], ref["ga"], ref["aux"], slope, gg, expect=want, grads=grads)
    three = launch(G, ref["y"], ref["ga"], ref["aux"], slope, gg, resident=False, grads=grads)
    for tag, r in (("resident", got), ("three-launch", three)):
        assert torch.equal(r["gy"], ref["gy"]), f"{tag} g_y: " + first_diff(r["gy"].float(), ref["gy"].float())
        assert torch.equal(r["sums"], ref["sums"]), f"{tag} sums (t1 | t2): " + first_diff(r["sums"], ref["sums"])
        if grads:
            assert torch.equal(r["dgamma"], ref["dgamma"]), f"{tag} dgamma: " + first_diff(r["dgamma"], ref["dgamma"])
            assert torch.equal(r["dbeta"], ref["dbeta"]), f"{tag} dbeta: " + first_diff(r["dbeta"], ref["dbeta"])


def test_every_instantiation_is_planned(G):
    """the exact table reaches every <NCH, NG> of the launcher's switch, by the plan its cases assert before they launch"""
    seen, missing = set(), []
    for nch, groups, c, *_ in EXACT:
        rows = tier_rows(G, nch, c)
        if rows is None:
            missing.append((nch, c))
            continue
        p = plan(G, rows, c, groups)
        assert p is not None and p[:2] == (nch, expected_ng(nch, groups)), (nch, groups, c, rows, p)
        seen.add(p[:2])
    if missing:
        pytest.skip(f"tiers (nch, C) out of reach with this chip's workgroup count: {missing}; planned {sorted(seen)}")
    assert seen == SWITCH, f"not planned: {sorted(SWITCH - seen)}, not in the switch: {sorted(seen - SWITCH)}"


# ---------------------------------------------------------------------------------------------------------------------
# (b), (c): true statistics, elementwise
# ---------------------------------------------------------------------------------------------------------------------
def slope32(slope):
    return float(torch.tensor(slope, dtype=torch.float32))


def group_reference(y, ga, gamma, beta, slope):
    """bn_ref.first_order of one group ([rows][C] fp64, storage-rounded) -> aux (fp32), g_y, its bound E, the sums and their bounds"""
    n = y.shape[0]
    f = bn_ref.first_order(y, ga, gamma, beta, slope32(slope))
    mean, invstd = f["mean"], 1.0 / f["sigma"]
    scale = gamma * invstd
    shift = beta - mean * scale
    aux = torch.cat([scale, shift, mean, invstd]).float()
    # the kernel's fp32 z must fall on the reference's side of 0
    zb = 4 * U * ((y * scale).abs() + shift.abs())
    same_zero = (y == 0) & (aux[y.shape[1]:2 * y.shape[1]] == 0)
    ambiguous = int(((f["z"].abs() <= zb) & ~(same_zero & (f["z"] == 0))).sum())
    assert ambiguous == 0, f"{ambiguous} elements have z within fp32 rounding of 0: the activation's branch is not determined"
    gza = f["gz"].abs()
    ya = y.abs() + mean.abs()
    w = gza * ya
    s_gz, s_w = gza.sum(0), w.sum(0)
    e = K_ELEM * U * scale.abs() * (gza + s_gz / n + ya * (invstd ** 2 * (s_w / n)))
    lim = min(n, L_SUM)
    return dict(aux=aux, gy=f["gy"], e=e, s1=f["sgz"], s2=f["sgzx"], b1=(lim + 1) * U * s_gz, b2=(lim + 6) * U * invstd * s_w,
                a1=s_gz, a2=invstd * s_w)


def elementwise_ratio(got, ref, e):
    """|got - ref| / (half a bf16 ulp of max(|got|, |ref|) + e), elementwise (fp64)"""
    got = got.double()
    big = torch.maximum(got.abs(), ref.abs())
    _, ex = torch.frexp(big)                                    # big = m 2^ex, 0.5 <= m < 1: ulp = 2^(ex - 8)
    half = torch.where(big > 0, torch.ldexp(torch.ones_like(big), ex - 9), torch.zeros_like(big))
    r = (got - ref).abs() / (half + e).clamp_min(1e-300)
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))


def assert_within(ratio, what):
    m = float(ratio.max())
    if not m <= 1.0:
        i = tuple(torch.nonzero(ratio == ratio.max())[0].tolist())
        raise AssertionError(f"{what}: error / bound = {m:.3g} at {i}; {int((ratio > 1).sum())} of {ratio.numel()} over the bound")
    return m


def build_stat_case(parts, slope, grad_groups):
    """parts: per group (y, ga, gamma, beta) in fp64, y / ga storage-rounded -> device inputs and the per-group references"""
    refs = [group_reference(y, ga, gamma, beta, slope) for y, ga, gamma, beta in parts]
    y = torch.stack([p[0] for p in parts]).bfloat16()
    ga = torch.stack([p[1] for p in parts]).bfloat16()
    aux = torch.stack([r["aux"] for r in refs])
    c = y.shape[2]
    dg, db = torch.full((c,), DG0, dtype=torch.float64), torch.full((c,), DB0, dtype=torch.float64)
    bg, bb = 4 * U * dg.abs(), 4 * U * db.abs()
    for r in refs[:grad_groups]:
        dg, db = dg + r["s2"], db + r["s1"]
        bg, bb = bg + r["b2"] + 4 * U * r["a2"], bb + r["b1"] + 4 * U * r["a1"]
    return dict(y=y, ga=ga, aux=aux, refs=refs, dgamma=dg, dbeta=db, bg=bg, bb=bb)


def check_stat_case(case, got, what, channels=None):
    """(b)'s criterion; channels: name -> index of the channels that are also compared on their own.  -> the worst ratios"""
    out = {}
    c = case["y"].shape[2]
    worst = 0.0
    per = {k: 0.0 for k in (channels or {})}
    s1w = s2w = 0.0
    for k, r in enumerate(case["refs"]):
        ratio = elementwise_ratio(got["gy"][k], r["gy"], r["e"])
        worst = max(worst, assert_within(ratio, f"{what} g_y, group {k}"))
        for name, ch in (channels or {}).items():
            per[name] = max(per[name], assert_within(ratio[:, ch], f"{what} g_y, group {k}, channel {name}"))
        s = got["sums"][k].double()
        s1w = max(s1w, assert_within((s[:c] - r["s1"]).abs() / r["b1"].clamp_min(1e-300), f"{what} sum g_z, group {k}"))
        s2w = max(s2w, assert_within((s[c:] - r["s2"]).abs() / r["b2"].clamp_min(1e-300), f"{what} sum g_z xhat, group {k}"))
    out.update(gy=worst, s1=s1w, s2=s2w, **per)
    if got["dgamma"] is not None:
        out["dgamma"] = assert_within((got["dgamma"].double() - case["dgamma"]).abs() / case["bg"], f"{what} dgamma")
        out["dbeta"] = assert_within((got["dbeta"].double() - case["dbeta"]).abs() / case["bb"], f"{what} dbeta")
    return out


def bf16_round(t):
    return t.float().bfloat16().double()


# (rows as a function of per_iter, C, groups, slope, grad_groups, the (nch, ng) it is meant for)
RAGGED = [("1", lambda p: 1, 512, 1, 0.2, 1, (1, 1)), ("3", lambda p: 3, 1024, 2, 0.0, 1, (1, 2)), ("63", lambda p: 63, 2048, 3, 0.2, 3, (1, 3)),
          ("64", lambda p: 64, 512, 1, 0.0, 0, (1, 1)), ("65", lambda p: 65, 1024, 2, 0.2, 2, (1, 2)),
          ("p-1", lambda p: p - 1, 512, 1, 0.2, 1, (1, 1)), ("p", lambda p: p, 256, 3, 0.0, 2, (1, 3)), ("p+1", lambda p: p + 1, 256, 2, 0.2, 1, (2, 2)),
          ("4p+37", lambda p: 4 * p + 37, 128, 3, 0.2, 2, (8, 2)), ("8p+5", lambda p: 8 * p + 5, 64, 3, 0.2, 2, (16, 1)),
          ("16p-1", lambda p: 16 * p - 1, 64, 2, 0.0, 1, (16, 1))]


@functools.lru_cache(maxsize=1)
def ragged_case(rows, c, groups, slope, grad_groups):
    parts = []
    for k in range(groups):
        inp = bn_ref.inputs(rows, c, seed=40 + k)
        parts.append((bf16_round(inp["y"]), bf16_round(inp["ga"]), inp["gamma"].float().double(), inp["beta"].float().double()))
    return build_stat_case(parts, slope, grad_groups)


@pytest.mark.parametrize("spec", RAGGED, ids=[s[0] for s in RAGGED])
def test_ragged_rows_true_statistics(G, spec):
    name, rows_of, c, groups, slope, gg, want = spec
    rows = rows_of(per_iter(G, c))
    case = ragged_case(rows, c, groups, slope, gg)
    what = f"{groups} x {rows} x {c}"
    got = launch(G, case["y"], case["ga"], case["aux"], slope, gg, expect=want)
    r = check_stat_case(case, got, what, {"neg": NEG, "small": SMALL})
    print(f"BNRESX ragged {name} {what} plan {want}: " + " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    again = launch(G, case["y"], case["ga"], case["aux"], slope, gg, expect=want, inplace=True)
    for key in ("gy", "sums", "dgamma", "dbeta"):
        assert same_bits(got[key], again[key]), f"{what}: {key} in place differs from out of place: " + first_diff(again[key].float(), got[key].float())


@functools.cache
def edge_case(rows, slope, grad_groups):
    c, parts = 64, []
    for k in range(3):
        inp = bn_ref.inputs(rows, c, seed=60 + k)
        y, gamma, beta = inp["y"], inp["gamma"].float().double(), inp["beta"].float().double()
        y[:, ZERO] = 0.0
        beta[ZERO] = 0.0
        if k == 1:
            y[:, JUMP] = y[:, JUMP] / 4 + 3            # the same xhat (and g_a's correlation with it), another mean and invstd
        parts.append((bf16_round(y), bf16_round(inp["ga"]), gamma, beta))
    case = build_stat_case(parts, slope, grad_groups)
    a = case["aux"].double()
    assert not a[:, 64 + ZERO].any() and not a[:, 128 + ZERO].any(), "the all-zero channel must have shift == 0 and mean == 0 exactly"
    for k in range(3):
        assert bool((case["refs"][k]["gy"][:, ZERO] == 0).all()) == (slope == 0.0) and not parts[k][0][:, ZERO].any()
    for other in (0, 2):                               # group 1's JUMP channel: mean about 3 away, invstd about 4 times the neighbours'
        assert abs(float(a[1, 128 + JUMP] - a[other, 128 + JUMP])) > 2.5 and 3.5 < float(a[1, 192 + JUMP] / a[other, 192 + JUMP]) < 4.5
    return case


def edge_rows(G):
    return 4 * per_iter(G, 64) + 37


@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_edge_channels(G, slope):
    rows, gg = edge_rows(G), 2
    case = edge_case(rows, slope, gg)
    got = launch(G, case["y"], case["ga"], case["aux"], slope, gg, expect=(8, 2))
    r = check_stat_case(case, got, f"edge channels, slope {slope}", DEDICATED)
    print(f"BNRESX edge slope {slope} 3 x {rows} x 64: " + " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    if slope == 0.0:                                   # ReLU'(0) = 0: nothing flows through the all-zero channel
        assert not got["gy"][:, :, ZERO].float().any() and not got["sums"][:, ZERO].any()
    else:                                              # LeakyReLU'(0) = slope
        assert bool((got["sums"][:, ZERO] != 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# (d) non-finite gradients
# ---------------------------------------------------------------------------------------------------------------------
@functools.cache
def clean_run(G, rows, grad_groups):
    case = edge_case(rows, 0.2, 2)                     # (c)'s tensor; grad_groups only changes which groups dgamma / dbeta sum
    return launch(G, case["y"], case["ga"], case["aux"], 0.2, grad_groups, expect=(8, 2))


@pytest.mark.parametrize("grad_groups", [1, 2])
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_non_finite_gradient(G, kind, grad_groups):
    rows, ch, grp = edge_rows(G), 7, 1
    case = edge_case(rows, 0.2, 2)
    clean = clean_run(G, rows, grad_groups)
    ga = case["ga"].clone()
    ga[grp, rows // 3, ch] = float(kind)
    got = launch(G, case["y"], ga, case["aux"], 0.2, grad_groups, expect=(8, 2))
    three = launch(G, case["y"], ga, case["aux"], 0.2, grad_groups, resident=False)
    what = f"one {kind} in g_a, grad_groups {grad_groups}"
    for tag, r in (("resident", got), ("three-launch", three)):
        assert not torch.isfinite(r["gy"][grp, :, ch].float()).any(), f"{what}, {tag}: finite g_y in the poisoned channel"
        assert not torch.isfinite(r["sums"][grp, [ch, 64 + ch]]).any(), f"{what}, {tag}: finite sums in the poisoned channel"
        for key in ("dgamma", "dbeta"):
            assert bool(torch.isfinite(r[key][ch])) == (not grp < grad_groups), f"{what}, {tag}: {key} = {float(r[key][ch])}"
    keep = torch.ones(3, 1, 64, dtype=torch.bool)
    keep[grp, 0, ch] = False
    gy_clean = torch.where(keep, clean["gy"], torch.zeros((), dtype=torch.bfloat16))
    gy_got = torch.where(keep, got["gy"], torch.zeros((), dtype=torch.bfloat16))
    assert same_bits(gy_got, gy_clean), f"{what}: g_y changed outside the poisoned channel: " + first_diff(gy_got.float(), gy_clean.float())
    keep_s = torch.ones(3, 128, dtype=torch.bool)
    keep_s[grp, ch] = keep_s[grp, 64 + ch] = False
    assert same_bits(torch.where(keep_s, got["sums"], torch.zeros(())), torch.where(keep_s, clean["sums"], torch.zeros(()))), f"{what}: other sums changed"
    others = [k for k in range(64) if k != ch]
    for key in ("dgamma", "dbeta"):
        assert same_bits(got[key][others], clean[key][others]), f"{what}: {key} of the other channels changed"
        if not grp < grad_groups:
            assert same_bits(got[key], clean[key]), f"{what}: {key} changed although group {grp} adds nothing to it"


# ---------------------------------------------------------------------------------------------------------------------
# (e) refusals and fallbacks
# ---------------------------------------------------------------------------------------------------------------------
def small_case(rows, c, groups, dtype=torch.bfloat16, seed=5):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(groups, rows, c, generator=g) * 1.5 + 0.3).to(dtype)
    aux = torch.empty(groups, 4 * c)
    xhat = torch.empty(groups, rows, c)
    for k in range(groups):
        yf = y[k].float()
        mean, invstd = yf.mean(0), 1.0 / torch.sqrt(yf.var(0, unbiased=False) + 1e-5)
        xhat[k] = (yf - mean) * invstd
        aux[k] = torch.cat([invstd, -mean * invstd, mean, invstd])
    ga = (0.6 * xhat + 0.5 + torch.randn(groups, rows, c, generator=g)).to(dtype)
    return y, ga, aux


def test_plan_refusals_and_fallbacks(G):
    p64 = per_iter(G, 64)
    small = min(2048, p64)
    assert plan(G, small, 64, 1) == (1, 1, plan(G, 1, 64, 1)[2])
    assert plan(G, small, 64, 1, prec=1) is None and plan(G, small, 64, 1, prec=2) is None, "only bf16 storage is resident"
    assert plan(G, 256, 32, 1) is None and plan(G, 256, 96, 1) is None
    assert plan(G, 16 * p64, 64, 1)[0] == 16 and plan(G, 16 * p64 + 1, 64, 1) is None
    p2048 = per_iter(G, 2048)
    over = 16 * p2048 + 1
    assert plan(G, over, 2048, 1) is None
    try:
        G.lib.jck_tune(b"bn_res", 0)
        assert plan(G, small, 64, 1) is None and plan(G, small, 64, 3) is None
        G.lib.jck_tune(b"bn_res", 1)
        assert plan(G, small, 64, 1) is not None, "one group is resident by default"
        assert plan(G, small, 64, 2) is None, "several groups under the 120 MB threshold go to the three launches by default"
        y, ga, aux = small_case(small, 64, 2)
        a, b = launch(G, y, ga, aux, 0.2, 1, expect=None), launch(G, y, ga, aux, 0.2, 1, resident=False)
        assert all(same_bits(a[k], b[k]) for k in a), "bn_res = 1, two small groups: not the three-launch bits"
    finally:
        G.lib.jck_tune(b"bn_res", 2)
    for rows, c, groups, dtype, prec in ((small, 64, 1, torch.float32, 1), (256, 32, 2, torch.bfloat16, 0), (over, 2048, 1, torch.bfloat16, 0)):
        y, ga, aux = small_case(rows, c, groups, dtype)
        a = launch(G, y, ga, aux, 0.2, 1, expect=None, prec=prec)
        b = launch(G, y, ga, aux, 0.2, 1, resident=False, prec=prec)
        assert all(same_bits(a[k], b[k]) for k in a), f"{groups} x {rows} x {c} prec {prec}: not the three-launch bits"
    y, ga, aux = small_case(256, 96, 1)                # not a power of two: no BatchNorm kernel takes it, and both entry points say so
    ea = launch(G, y, ga, aux, 0.2, 1, expect=None, raises=True)
    eb = launch(G, y, ga, aux, 0.2, 1, resident=False, raises=True)
    assert ea == eb and "power of two" in ea, (ea, eb)
