"""The step engine's state BETWEEN two training steps, with the forward half of the next step's D(real) pass already enqueued.

step_async(next_real=...) (the default of a one-GPU trainer) leaves live state behind when it returns: real_noisy, group 0 of the
batched activation set, the engine's note of the step whose D(real) forward has run (with its event on the weight-gradient
stream), the next step's set-step launch (its z / alpha, cleared accumulator rows and cleared D gradients) and a BatchNorm record
slot of the next step's parity.  Every call made before the next step_async runs on top of that.  Three families of tests, all bit
for bit (the engine is deterministic: tests/test_score_gpu.py::test_score_between_two_training_steps_changes_no_bit is the pattern):

1. calls that must not change the run: the run with the call equals the run without it, and the call's own result equals that of
   the same call on a second engine that shares nothing with the first (loaded from state_dicts() and the Adam state at that point);
2. calls that change the weights: the run that announces every next batch equals the run that announces none - the prefetch is an
   optimisation, never another result;
3. transplant: a fresh engine given the state dicts, the Adam state (with t), the average and the noise seed of a running one
   continues that run.

Every announced run asserts that the prefetch was really recorded, so a silently disabled prefetch cannot make a test vacuous."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, LR, SEED = 8, 2e-4, 77
EMA = dict(ema_decay=0.9, ema_start=2)
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _state(family):
    def make():
        from oracle.gan_oracle import build_params
        torch.manual_seed(12345)
        return build_params(family)
    return _once(("params", family), make)


def _data():
    """(images of four steps, their one-hot labels) on the device"""
    def make():
        from util import synth_images, synth_onehot
        return synth_images(B * 4).cuda(), synth_onehot(B * 4)[0].cuda()
    return _once("data", make)


def _gp_inputs():
    """real / fake / alpha (and CGAN's labels and Dropout keep-mask) of a penalty call: NOT a batch of the run, so that a
    real_noisy it leaves behind differs from the one the next step needs"""
    def make():
        from util import synth_images, synth_onehot
        g = torch.Generator().manual_seed(31)
        fake = torch.randn(B, 3, 64, 64, generator=g).clamp_(-1, 1)
        alpha, mask = torch.rand(B, generator=g), (torch.rand(B, 256, generator=g) >= 0.25).float()
        return synth_images(B, seed=99).cuda(), fake.cuda(), alpha.cuda(), synth_onehot(B, seed=98)[0].cuda(), mask.cuda()
    return _once("gp", make)


def _new(family, prec, batch=B, **kw):
    from hipgan.engine import CganEngine, DcganEngine
    return (CganEngine if family == "cgan" else DcganEngine)(batch=batch, prec=prec, device="cuda:0", **kw)


def _pre(eng):
    """the key of the batch whose D(real) forward this engine has announced and enqueued, or None"""
    return getattr(eng, "_prefetched_real", None)


def _adam(eng, tag, named=True):
    """the optimiser view of one network's Adam state: its tensors by name for state_dict() / load_state_dict(); named=False for
    step(), which then has no module parameters to gather - the arenas are the state"""
    from hipgan.optim import EngineAdam
    return EngineAdam(eng, tag, [(k, None) for k in eng.named_views(tag, "m")] if named else [], LR, betas=[0.5, 0.999])


def _twin(eng):
    """A fresh engine that shares nothing with `eng`, given what a checkpoint holds of it: both state dicts, Adam's m / v / t of both
    networks through the optimiser's state dict, the average where one is kept, and the noise seed of these runs."""
    twin = _new("cgan" if eng.family == 1 else "dcgan", eng.prec, gp_backward=eng.gp_backward, ema_decay=eng.ema_decay or 0.0,
                ema_start=eng.ema_start)
    twin.load_state(*eng.state_dicts())
    for tag in ("g", "d"):
        _adam(twin, tag).load_state_dict(_adam(eng, tag).state_dict())
    if eng.ema_decay is not None:
        twin.load_ema_state(eng.ema_state_dict())
    twin.set_noise_seed(SEED)
    assert twin.t == eng.t and twin.arenas is not eng.arenas and twin.workspace.data_ptr() != eng.workspace.data_ptr()
    return twin


def _drive(eng, first, stop, announce, between=None, generator=None):
    """steps [first, stop) of the run on `eng`: between(eng, s) after step s and before step s + 1, scalars() after that.
    -> the scalars of those steps"""
    imgs, onehot = _data()
    scal = []
    for s in range(first, stop):
        kw = dict(next_real=imgs[(s + 1) * B:(s + 2) * B]) if announce and s + 1 < stop else {}
        if eng.family == 1:
            kw["labels"] = onehot[s * B:(s + 1) * B]
        eng.step_async(imgs[s * B:(s + 1) * B], None, LR, generator=generator, **kw)
        if "next_real" in kw:
            assert _pre(eng) is not None, "the announced batch was not prefetched: the test would check nothing"
        else:
            assert _pre(eng) is None
        if between is not None and s + 1 < stop:
            between(eng, s)
        scal.append(eng.scalars())
    return scal


def run(between=None, announce=False, graphs=False, prec="bf16", family="dcgan", steps=None, **engine_kw):
    """One training run (B = 8, 3 steps eager / 4 under graph replay, whose first step runs eagerly) with between(eng, s) after
    step s and before step s + 1.  -> (scalars per step, a clone of every arena)"""
    assert not (announce and (graphs or family == "cgan")), "graph replay and CGAN take no prefetch"
    steps = steps or (4 if graphs else 3)
    eng = _new(family, prec, **engine_kw)
    eng.graphs = graphs
    eng.load_state(*_state(family))
    eng.set_noise_seed(SEED)
    scal = _drive(eng, 0, steps, announce, between, torch.Generator(device="cuda").manual_seed(5))
    eng.join()
    torch.cuda.synchronize()
    assert (len(eng._graph_cache) > 0) == graphs
    return scal, {k: v.clone() for k, v in eng.arenas.items()}


def base(announce=False, graphs=False, prec="bf16", family="dcgan", **engine_kw):
    """the run with no call between its steps: computed once per configuration, never modified"""
    key = ("base", announce, graphs, prec, family, tuple(sorted(engine_kw.items())))
    return _once(key, lambda: run(None, announce, graphs, prec, family, **engine_kw))


def _expect_same(a, b, what, skip=()):
    assert len(a[0]) == len(b[0]) and set(a[1]) == set(b[1]), what
    for s, (x, y) in enumerate(zip(a[0], b[0])):
        assert x == y, f"{what}: scalars of step {s + 1}: {x} vs {y}"
    bad = [k for k in a[1] if k not in skip and not torch.equal(a[1][k], b[1][k])]
    assert not bad, f"{what}: arenas differ: {bad}"


def _differs(a, b):
    return a[0] != b[0] and any(not torch.equal(a[1][k], b[1][k]) for k in a[1])


def _same(x, y):
    """nested dicts / lists of tensors and numbers: equal bit for bit"""
    if isinstance(x, dict):
        return isinstance(y, dict) and list(x) == list(y) and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(_same(p, q) for p, q in zip(x, y))
    if torch.is_tensor(x):
        return torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())
    return x == y


def test_the_prefetch_itself_changes_no_bit():
    """what every comparison below rests on: announcing the next batch is the same run (bf16, f32, with the average)"""
    for kw in (dict(prec="bf16"), dict(prec="f32"), dict(prec="bf16", **EMA)):
        _expect_same(base(True, **kw), base(False, **kw), f"announced vs not {kw}")
    assert _differs(base(prec="bf16"), base(prec="f32"))


# ---------------------------------------------------------------------------------------------------------------------
# 1. calls that must not change the run
# ---------------------------------------------------------------------------------------------------------------------
def _gp_between(announce, calls):
    def between(eng, s):
        real, fake, alpha, lab, mask = _gp_inputs()
        extra = (lab, mask) if eng.family == 1 else ()
        norms = eng.gradient_penalty_pass(real, fake, alpha, *extra).clone()
        dgr = eng.arenas["d_grads"].clone() if eng.gp_backward else None
        # the announced batch is still this engine's next real batch (whether its prefetched pass was kept or is computed again)
        assert (_pre(eng) is not None) == announce
        twin = _twin(eng)
        ref = twin.gradient_penalty_pass(real, fake, alpha, *extra)
        assert bool(torch.isfinite(norms).all()) and float(norms.min()) > 0.0
        assert torch.equal(norms, ref), f"norms after step {s + 1}: {norms.tolist()} vs {ref.tolist()}"
        if dgr is not None:
            assert float(dgr.abs().max()) > 0.0 and torch.equal(dgr, twin.arenas["d_grads"]), f"d_grads after step {s + 1}"
        calls.append(s)
    return between


GP_CASES = [pytest.param(dict(prec=p), a, id=f"dcgan-{p}-{'announced' if a else 'plain'}") for p in ("bf16", "f32") for a in (True, False)]
GP_CASES += [pytest.param(dict(prec="bf16", graphs=True), False, id="dcgan-bf16-graph"),
             pytest.param(dict(prec="bf16", gp_backward=True), True, id="dcgan-bf16-gp_backward-announced"),
             pytest.param(dict(prec="bf16", family="cgan"), False, id="cgan-bf16")]


@pytest.mark.parametrize("kw,announce", GP_CASES)
def test_gradient_penalty_pass_between_two_steps(kw, announce):
    """Engine.gradient_penalty_pass (PHASE_GP_ONLY) on the training engine, on images that are not the announced batch: the norms
    (and, where the penalty is back-propagated, D's gradient arena right after the call) are those of an engine that shares
    nothing, and the run goes on as if the call had not been made - the scalars read right after the call are still the previous
    step's (the call clears accumulator rows of the next step's parity only), the gradients it leaves are cleared by the next
    step, and the next step's conv1 weight gradient sees the noisy real batch, not the call's `real`."""
    calls = []
    got = run(_gp_between(announce, calls), announce, **kw)
    assert len(calls) == len(got[0]) - 1
    _expect_same(got, base(announce, **kw), f"gradient_penalty_pass {kw}")


def test_gradient_penalty_pass_keeps_the_steps_inputs_alive():
    """the tensors the step in flight still reads (its real batch, the announced one) stay referenced across the call"""
    def between(eng, s):
        before = list(eng._keep)
        assert before
        eng.gradient_penalty_pass(*_gp_inputs()[:3])
        assert all(any(t is u for u in eng._keep) for t in before)
    run(between, True)


def _z(n, seed):
    return torch.randn(n, 100, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("out", ["float", "uint8"])
def test_sample_running_between_two_steps(out):
    """eval-mode sampling on the training engine: any n (13 = two chunks), nothing written"""
    z = _z(13, 21)

    def between(eng, s):
        img = eng.sample(z, bn="running", out=out)
        assert _pre(eng) is not None
        ref = _twin(eng).sample(z, bn="running", out=out)
        assert img.dtype == (torch.uint8 if out == "uint8" else torch.float32) and float(img.float().std()) > 0.0
        assert torch.equal(img, ref), f"sample after step {s + 1}"
    _expect_same(run(between, True), base(True), f"sample(bn='running', out={out!r})")


def test_sampling_the_average_between_two_steps():
    """train-mode sampling of the averaged generator on its sampling engine (a workspace of its own on the same arenas): it moves
    g_ema_bn / g_ema_nbt and nothing else"""
    z = _z(B, 22)

    def between(eng, s):
        if s == 0:
            eng.smp = _new("dcgan", "bf16", share=eng, ema=True)
        nbt = eng.arenas["g_ema_nbt"].clone()
        img = eng.smp.sample(z, bn="batch")
        assert _pre(eng) is not None
        assert bool((eng.arenas["g_ema_nbt"] != nbt).any())
        twin = _twin(eng)
        ref = _new("dcgan", "bf16", share=twin, ema=True).sample(z, bn="batch")
        assert float(img.std()) > 0.0 and torch.equal(img, ref), f"sample of the average after step {s + 1}"
    got = run(between, True, **EMA)
    _expect_same(got, base(True, **EMA), "ema sampling engine", skip=("g_ema_bn", "g_ema_nbt"))
    assert not torch.equal(got[1]["g_ema_bn"], base(True, **EMA)[1]["g_ema_bn"])


def test_snapshots_between_two_steps():
    """state_dicts(), ema_state_dict(), both optimisers' state dicts, tensor("real_noisy") and record_scalars(): what they return with
    a prefetch in flight is what they return at the same point of the run that announced nothing, and the run is unchanged.
    (tensor("real_noisy") legitimately shows the NEXT batch while a prefetch is in flight: its content is not compared.)"""
    snaps = {True: [], False: []}

    def between_for(announce):
        def between(eng, s):
            row = torch.full((8,), -7.0, device="cuda")
            eng.record_scalars(row)
            snap = {"sd": eng.state_dicts(), "ema": eng.ema_state_dict(), "opt_g": _adam(eng, "g").state_dict(),
                    "opt_d": _adam(eng, "d").state_dict(), "row": row.cpu()}
            assert eng.tensor("real_noisy").numel() == B * 64 * 64 * 4
            assert (_pre(eng) is not None) == announce
            assert snap["row"].tolist() == list(eng.scalars().values())
            assert float(snap["opt_d"]["state"][0]["step"]) == s + 1 and float(snap["opt_d"]["state"][0]["exp_avg"].abs().max()) > 0.0
            snaps[announce].append(snap)
        return between
    for announce in (True, False):
        _expect_same(run(between_for(announce), announce, **EMA), base(announce, **EMA), f"snapshots, announced={announce}")
    assert len(snaps[True]) == 2 and _same(snaps[True], snaps[False])
    assert not _same(snaps[True][0], snaps[True][1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. calls that change the weights: announced equals not announced
# ---------------------------------------------------------------------------------------------------------------------
def _both(between, what, **kw):
    """the run with `between`, once with every next batch announced and once with none: equal.  -> that run"""
    a, b = run(between, True, **kw), run(between, False, **kw)
    _expect_same(a, b, f"{what}: announced vs not announced")
    return a


def _dropped(eng):
    assert _pre(eng) is None, "mark_weights_changed left the prefetch recorded"


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_identity_reload_between_two_steps(prec):
    """load_state(*state_dicts()) drops the prefetched pass (computed with operands about to be re-derived) and is the same run"""
    def between(eng, s):
        eng.load_state(*eng.state_dicts())
        _dropped(eng)
    _expect_same(_both(between, "identity reload", prec=prec), base(False, prec=prec), "identity reload vs none")


def test_identity_reload_with_the_average_restored():
    """load_state resets the average to the weights; load_ema_state(ema_state_dict()) from before puts it back: g_ema included"""
    def between(eng, s):
        ema = eng.ema_state_dict()
        eng.load_state(*eng.state_dicts())
        eng.load_ema_state(ema)
        _dropped(eng)
    got = _both(between, "identity reload + average", **EMA)
    _expect_same(got, base(False, **EMA), "identity reload + average vs none")
    assert not torch.equal(got[1]["g_ema"], got[1]["g_params"])


def test_weight_change_between_two_steps():
    """what the replica guard's re-broadcast does: an out-of-engine write to D's weights, then mark_weights_changed()"""
    def between(eng, s):
        eng.join()
        eng.arenas["d_params"][7] += 1e-3
        eng.mark_weights_changed()
        _dropped(eng)
    assert _differs(_both(between, "d_params[7] += 1e-3"), base(False)), "the perturbed run equals the unperturbed one"


def test_module_path_adam_step_between_two_steps():
    """EngineAdam(eng, "d").step() on a gradient arena filled with a fixed pattern"""
    def between(eng, s):
        n = eng.arenas["d_grads"].numel()
        pat = _once(("pattern", n), lambda: torch.randn(n, generator=torch.Generator().manual_seed(41)).cuda() * 1e-3)
        eng.join()
        eng.arenas["d_grads"].copy_(pat)
        before = eng.arenas["d_params"].clone()
        _adam(eng, "d", named=False).step()
        _dropped(eng)
        assert not torch.equal(eng.arenas["d_params"], before)
    assert _differs(_both(between, "EngineAdam.step"), base(False)), "the perturbed run equals the unperturbed one"


def test_sample_batch_between_two_steps():
    """train-mode sampling on the training engine moves g_bn / g_nbt and touches nothing of D: the prefetched pass survives"""
    z = _z(B, 23)

    def between(eng, s):
        pre = _pre(eng)
        img = eng.sample(z, bn="batch")
        assert _pre(eng) == pre
        assert bool(torch.isfinite(img).all()) and float(img.std()) > 0.0
    got = _both(between, "sample(bn='batch')")
    assert not torch.equal(got[1]["g_bn"], base(False)[1]["g_bn"]) and not torch.equal(got[1]["g_nbt"], base(False)[1]["g_nbt"])


def test_shared_ragged_engine_steps_between_two_steps():
    """A share= engine at batch 6 (the per-pass schedule; an epoch's ragged tail) takes one step between two steps of the main
    engine, which had announced its next batch: the main engine's prefetched D(real) forward was computed with the weights of
    before that step and must not be consumed.  The reference run announces nothing.  (That step also advances the step count the
    engines share, so the native engine's note of the prefetched step no longer matches the next step and it computes D(real)
    itself; the case below moves the version alone.)"""
    from util import synth_images
    tail_imgs = synth_images(6, seed=97).cuda()

    def between(eng, s):
        if s == 0:
            eng.tail = _new("dcgan", "bf16", batch=6, share=eng)
            eng.tail.set_noise_seed(4242)
        pre, t = _pre(eng), eng.t
        eng.tail.step_async(tail_imgs, None, LR)
        assert eng.t == t + 1 and _pre(eng) == pre     # the announced batch is still required
    assert _differs(_both(between, "share= engine's step"), base(False)), "the tail engine's steps changed nothing"


def test_weight_change_marked_on_a_shared_engine():
    """The same out-of-engine write, announced to a share= engine's mark_weights_changed() (whoever holds the arenas may be the one
    that writes them: a sampling engine's load_ema_state, an optimiser bound to the ragged engine).  The shared weight version
    moves but the step count does not, so only step_async's own look at the version keeps the main engine from consuming the
    D(real) forward it computed with the old weights."""
    def between(eng, s):
        if s == 0:
            eng.tail = _new("dcgan", "bf16", batch=6, share=eng)
        pre = _pre(eng)
        eng.join()
        eng.arenas["d_params"][7] += 1e-3
        eng.tail.mark_weights_changed()
        assert _pre(eng) == pre                             # the announced batch is still required
    got = _both(between, "d_params[7] += 1e-3 marked on a share= engine")
    assert _differs(got, base(False)), "the perturbed run equals the unperturbed one"


# ---------------------------------------------------------------------------------------------------------------------
# 3. transplant
# ---------------------------------------------------------------------------------------------------------------------
TRANSPLANT = [pytest.param(k, dict(kw), id=f"{i}-k{k}") for k in (1, 2) for i, kw in
              (("dcgan-bf16", dict(prec="bf16")), ("dcgan-f32", dict(prec="f32")), ("dcgan-bf16-ema", dict(prec="bf16", **EMA)),
               ("cgan-bf16", dict(prec="bf16", family="cgan")))]
TRANSPLANT += [pytest.param(2, dict(prec="bf16", announce=True), id="dcgan-bf16-announced-k2"),
               pytest.param(1, dict(prec="bf16", graphs_b=True), id="dcgan-bf16-graph-k1")]


@pytest.mark.parametrize("k,kw", TRANSPLANT)
def test_transplant_continues_the_run(k, kw):
    """k steps on engine A, its state moved into a fresh engine B (_twin: state dicts, Adam's m / v / t through the optimisers' state
    dicts, the average, the noise seed), n = 2 more steps on B with the engine's own draws: scalars of steps k+1..k+n and every arena
    equal those of A running k+n steps without a break.  B starts on either step parity with none of the step's promises (cleared
    accumulator rows, cleared gradients, z in place) made.  announce: A's state is taken with a prefetch in flight and B goes on
    announcing; graphs_b: B replays its second step from a captured graph."""
    n, announce, graphs_b = 2, kw.pop("announce", False), kw.pop("graphs_b", False)
    twins = []

    def between(eng, s):
        assert eng.fast_noise
        if s == k - 1:
            twins.append(_twin(eng))
    a = run(between, announce, steps=k + n, **kw)
    b_eng, = twins
    b_eng.graphs = graphs_b
    scal = _drive(b_eng, k, k + n, announce)
    b_eng.join()
    torch.cuda.synchronize()
    assert (len(b_eng._graph_cache) > 0) == graphs_b and b_eng.t == k + n
    _expect_same((a[0][k:], a[1]), (scal, {key: v.clone() for key, v in b_eng.arenas.items()}), f"transplant after step {k} {kw}")
