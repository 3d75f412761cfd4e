"""-m gpu: the frozen teacher's cloning term at the library level (hgym_guide_schedule, hgym_ppo_grad_guide) against
tests/guidance_common.py's float64 reference.

1. hgym_guide_schedule against its Python twin, exact, at the edges of every mode and at 2^40; the count advances by one per launch.
2. The gradient and the sum on all three paths of U.PATHS at U.SHAPES (fp32 rows and the bf16 shadow, ELU(1) and Tanh, both value-loss
   forms, log std, the auxiliary head, normalisation) at the project's bars; everything but the actor's gradient torch.equal
   hgym_ppo_grad's on the same inputs; the coefficient comes from hgym_guide_schedule at update K.
3. On the fused path also at B = 1, 63, 64, 65, 200 with fp32 rows and the bf16 shadow under ELU(1) and Tanh.
4. With the device coefficient 0.0 everything torch.equal hgym_ppo_grad's; the squared error is still reported.
5. The coefficient is read from the device: the same call twice with only the device float changed gives the two references' gradients.
6. The same bits from a second call (the sums are added in a fixed order).
7. One optimiser step moves the actor toward the teacher.
8. Misuse is refused with HGYM_E_BADARG and nothing written."""
import ctypes as C

import pytest
import torch

import guidance_common as GC
import update_options_common as U
import test_update_options_gpu as G
from hgym import _lib as L

pytestmark = pytest.mark.gpu

O = U.Options
FUSED = [O("bf16-fused", act, "scalar", vu, False, False, sh) for act in (None, U.TANH) for vu in (False, True) for sh in (False, True)]
LAYER = [O(p, act, "scalar", False, False, False, False) for p in ("f32-layer", "bf16-layer") for act in (None, U.TANH)]
EXTRA = [O("bf16-fused", None, "log", False, False, False, True), O("bf16-fused", None, "scalar", False, True, False, True),
         O("bf16-fused", U.TANH, "log", True, True, True, False), O("f32-layer", None, "scalar", True, False, True, False),
         O("bf16-layer", None, "log", True, True, True, False)]
CASES = FUSED + LAYER + EXTRA
ALONE = [O(p, None, "scalar", False, False, False, p == "bf16-fused") for p in U.PATHS]
EDGES = (1, 63, 64, 65, 200)

_BIG = {}


def _net_for(opts, B):
    """G._net's NetBuffers, or -- a fused minibatch of more than its 128 rows -- one of the same shape with room for 256."""
    if B <= 128:
        return G._net(opts)
    from hgym import NetBuffers, make_net_config
    key = (opts.activation is not None, opts.std)
    if key not in _BIG:
        no, npv, A, ah, ch = U.SHAPES[opts.path]["net"]
        cfg = make_net_config(no, npv, A, ah, ch, "bf16", 256, activation=opts.activation, fused_activation=True, noise_std_type=opts.std)
        _BIG[key] = NetBuffers(cfg, "cuda", learning_rate=G.LR)
        assert _BIG[key].shadow_ld(0) > 0
    net = _BIG[key]
    for t in (net.adam_m, net.adam_v, net.opt_state, net.grads_ext):
        t.zero_()
    net.opt_state[L.OPT_LR] = G.LR
    return net


# ---------------------------------------------------------------------------------------------- 1. the schedule
def test_schedule_against_the_python_twin():
    import hgym
    i0, i1 = 8, 24
    scheds = [hgym.make_guide_schedule("linear", 0.75, 0.125, i0, i1), hgym.make_guide_schedule("step", 0.75, 0.125, final_step=i1),
              hgym.make_guide_schedule("constant", 0.75), hgym.make_guide_schedule("linear", 0.1, 0.0, 0, 3),
              hgym.make_guide_schedule("linear", 0.3, 0.7, 5, 12), GC.sched()]
    edges = (0, 1, 2, 3, i0 - 1, i0, (i0 + i1) // 2, i1 - 1, i1, i1 + 1, 2 ** 40)
    count = torch.zeros(3, dtype=torch.int64, device="cuda")
    coef = torch.full((3,), float("nan"), device="cuda")
    for s in scheds:
        for k in edges:
            count[0] = k
            hgym.guide_schedule(s, count, coef)
            hgym.guide_schedule(s, count, coef[1:])      # the next update's, from the advanced count
            torch.cuda.synchronize()
            got = coef.cpu()
            assert float(got[0]) == hgym.guide_schedule_coef(s, k), (s.mode, k, float(got[0]))
            assert float(got[1]) == hgym.guide_schedule_coef(s, k + 1), (s.mode, k)
            assert int(count[0]) == k + 2 and int(count[1]) == 0 and bool(torch.isnan(coef[2]))


# ---------------------------------------------------------------------------------------------- 2. the gradient
def _grad(net, opts, case, ppo, shadow, coef=None, plain=False, k=GC.K, teacher=None):
    """One hgym_ppo_grad_guide (plain: hgym_ppo_grad) + the unfold on the case.  The coefficient: hgym_guide_schedule of GC.sched() at
    update k, or the float `coef` planted.  -> (sums, the device coefficient, the update count)."""
    import hgym
    cols = [t.cuda().contiguous() for t in case["cols"]]
    kw = {}
    if shadow:
        sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(torch.bfloat16).cuda().contiguous()
        kw = dict(obs_bf16=sh(case["cols"][0], net.shadow_ld(0)), priv_bf16=sh(case["cols"][1], net.shadow_ld(1)))
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    count = torch.full((1,), k, dtype=torch.int64, device="cuda")
    c = torch.full((1,), float("nan"), device="cuda")
    tmu = (case["teacher_mu"] if teacher is None else teacher).cuda().contiguous()
    net.opt_state[L.OPT_KL_SUM:L.OPT_MINIBATCHES + 1] = 0.0
    net.opt_state[L.OPT_KL_LAST:L.OPT_AUX_SUM + 1] = 0.0
    idx = case["idx"].cuda()      # (held: the batch descriptor carries its address, not the tensor)
    batch = hgym.make_batch(*cols, idx, **kw)
    if plain:
        net.ppo_grad(ppo, batch)
    else:
        if coef is None:
            hgym.guide_schedule(GC.sched(), count, c)
        else:
            c.fill_(coef)
        net.ppo_grad_guide(ppo, batch, hgym.make_guide(tmu, c, sums))
    if opts.norm:
        net.norm_unfold_grad()
    torch.cuda.synchronize()
    return sums.cpu(), float(c), int(count)


_hold = G._hold
OPT_KEPT = (L.OPT_LR, L.OPT_STEP, L.OPT_KL_SUM, L.OPT_SURROGATE_SUM, L.OPT_VALUE_SUM, L.OPT_ENTROPY_SUM, L.OPT_MINIBATCHES, L.OPT_KL_LAST,
            L.OPT_AUX_SUM)


def _others_keep_their_bits(net, g0, o0, actor_too=False):
    """Everything but the actor's gradient -- d std, the critic, the auxiliary head, the KL slot, the loss sums -- against the plain run;
    actor_too: the actor's gradient as well (torch.equal: the value, a zero's sign aside)."""
    views, base = net.views, net.params.data_ptr()
    flat0, flat1 = g0[:net.P], net.grads_ext[:net.P]
    moved = 0
    for k, v in views.items():
        o = (v.data_ptr() - base) // 4
        a, b = flat0[o:o + v.numel()], flat1[o:o + v.numel()]
        if k.startswith("actor."):
            moved += int(not torch.equal(a, b))
        else:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s moved with the term on" % k
    assert moved == (0 if actor_too else len([k for k in views if k.startswith("actor.")])), moved
    assert torch.equal(g0[net.P:].view(torch.int32), net.grads_ext[net.P:].view(torch.int32))      # the KL slot
    for slot in OPT_KEPT:
        assert float(o0[slot]) == float(net.opt_state[slot]), slot


def _check(opts, case, shadow, report=True):
    net = _net_for(opts, case["B"])
    G._load(net, opts, case)
    ppo = G._ppo(opts, case)
    _grad(net, opts, case, ppo, shadow, plain=True)
    g0, o0 = net.grads_ext.clone(), net.opt_state.clone()
    sums, c, count = _grad(net, opts, case, ppo, shadow)
    assert c == GC.coef_at(GC.K) and count == GC.K + 1      # the schedule's value on the device is the twin's
    assert torch.isfinite(net.grads_ext).all()
    ref = GC.reference(case)
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    what = "guidance c=%g B=%d %s" % (c, case["B"], U.case_id(opts))
    _hold("%s: gradient vs float64 reference" % what, opts, U.errors(opts, got, ref), U.bar_of(opts), report=report)
    _hold("%s: loss sums" % what, opts, U.sum_errors(opts, G._sums(net), ref), U.SUM_TOL[opts.path], report=report)
    err = abs(float(sums[0]) - ref["guide"]) / ref["guide"]
    print("    sums[0] %.6e vs %.6e: rel %.3e (bar %.1e)" % (float(sums[0]), ref["guide"], err, U.SUM_TOL[opts.path]))
    assert err <= U.SUM_TOL[opts.path] and float(sums[1]) == 1.0
    _others_keep_their_bits(net, g0, o0)
    return net, ppo


@pytest.mark.parametrize("opts", CASES, ids=[U.case_id(o) for o in CASES])
def test_gradient_and_sum_of_every_instantiation(opts):
    case = GC.case_of(opts)
    net, ppo = _check(opts, case, opts.shadow)
    if opts.shadow:      # the bf16 shadow rows and the fp32 rows give the same bits
        ext = net.grads_ext.clone()
        _grad(net, opts, case, ppo, False)
        assert torch.equal(ext.view(torch.int32), net.grads_ext.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 3. batch edges
@pytest.mark.parametrize("shadow", [False, True], ids=["fp32rows", "shadow"])
@pytest.mark.parametrize("act", [None, U.TANH], ids=["elu", "tanh"])
@pytest.mark.parametrize("B", EDGES)
def test_fused_batch_edges(B, act, shadow):
    # (unclipped: one row's d V is never 0, so the last critic bias's metric -- against ||d_val|| -- is defined at B = 1; the actor's head,
    # which is what these cases are about, is the same kernel under either value loss)
    opts = O("bf16-fused", act, "scalar", True, False, False, shadow)
    case = GC.make_case(opts._replace(shadow=False), seed=60 + B, B=B) if B <= 128 else _big_case(opts)
    _check(opts, case, shadow, report=False)


def _big_case(opts, _cache={}):
    key = opts.activation is not None
    if key not in _cache:      # 260 stored rows, 200 drawn: four update tiles, the last with 8 rows
        o = opts._replace(shadow=False)
        c = U.make_case(o, S=260, B=200, seed=260)
        g = torch.Generator().manual_seed(GC.TEACHER_SEED + 260)
        mu_t, _, _ = U.forward(o, U.make_params(o, g), c["stats"], c["cols"][0], c["cols"][1])
        _cache[key] = dict(c, teacher_mu=mu_t.float().contiguous())
    return _cache[key]


@pytest.mark.parametrize("path", ["f32-layer", "bf16-layer"])
def test_layer_batch_edges(path):
    opts = O(path, None, "scalar", True, False, False, False)      # (unclipped: one row's d V is never 0, the last critic bias's metric is defined)
    for B in (1, 31):
        _check(opts, GC.make_case(opts, seed=80 + B, B=B), False, report=False)


# ---------------------------------------------------------------------------------------------- 4. coefficient 0
@pytest.mark.parametrize("opts", ALONE + [FUSED[5], LAYER[1], LAYER[3]], ids=[U.case_id(o) for o in ALONE + [FUSED[5], LAYER[1], LAYER[3]]])
def test_coefficient_zero_is_the_plain_update(opts):
    case = GC.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case)
    _grad(net, opts, case, ppo, opts.shadow, plain=True)
    g0, o0 = net.grads_ext.clone(), net.opt_state.clone()
    sums, c, _ = _grad(net, opts, case, ppo, opts.shadow, coef=0.0)
    assert c == 0.0
    assert torch.equal(g0, net.grads_ext)
    _others_keep_their_bits(net, g0, o0, actor_too=True)
    ref = GC.reference(case, c=0.0)
    assert abs(float(sums[0]) - ref["guide"]) / ref["guide"] <= U.SUM_TOL[opts.path] and float(sums[1]) == 1.0      # the error is still reported
    # ... and so is the schedule's 0 once it has run out
    sums, c, count = _grad(net, opts, case, ppo, opts.shadow, k=GC.FINAL)
    assert c == 0.0 and count == GC.FINAL + 1 and torch.equal(g0, net.grads_ext)


# ---------------------------------------------------------------------------------------------- 5. the coefficient is read from the device
@pytest.mark.parametrize("opts", ALONE + [FUSED[4]], ids=[U.case_id(o) for o in ALONE + [FUSED[4]]])
def test_coefficient_is_read_from_the_device(opts):
    """ONE HgymGuide, one batch: between the two calls only the device float changes."""
    import hgym
    case = GC.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case)
    cols = [t.cuda().contiguous() for t in case["cols"]]
    kw = {}
    if opts.shadow:
        sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(torch.bfloat16).cuda().contiguous()
        kw = dict(obs_bf16=sh(case["cols"][0], net.shadow_ld(0)), priv_bf16=sh(case["cols"][1], net.shadow_ld(1)))
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    c = torch.zeros(1, device="cuda")
    tmu = case["teacher_mu"].cuda()
    idx = case["idx"].cuda()      # (held: the batch descriptor carries its address, not the tensor)
    batch, guide, sched = hgym.make_batch(*cols, idx, **kw), hgym.make_guide(tmu, c, sums), GC.sched()
    seen = []
    for k in range(3):      # updates 0, 1, 2 of the schedule, as a captured update would run them
        net.opt_state[L.OPT_KL_SUM:L.OPT_MINIBATCHES + 1] = 0.0
        net.opt_state[L.OPT_KL_LAST:L.OPT_AUX_SUM + 1] = 0.0
        hgym.guide_schedule(sched, count, c)
        net.ppo_grad_guide(ppo, batch, guide)
        torch.cuda.synchronize()
        assert float(c) == GC.coef_at(k)
        got = {n: v.cpu() for n, v in net.grad_views().items()}
        ref = GC.reference(case, c=GC.coef_at(k))
        _hold("guidance update %d (c=%g) %s" % (k, float(c), U.case_id(opts)), opts, U.errors(opts, got, ref), U.bar_of(opts), report=False)
        seen.append(got)
        for other in range(3):      # ... and it is not another update's gradient
            if other != k:
                wrong = U.errors(opts, got, GC.reference(case, c=GC.coef_at(other)), names=[n for n in got if n.startswith("actor.")])
                assert max(wrong.values()) > U.bar_of(opts), (k, other, wrong)
    assert float(sums[1]) == 3.0 and int(count) == 3


# ---------------------------------------------------------------------------------------------- 6. the same bits every run
@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_same_bits_from_a_second_call(opts):
    case = GC.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case)
    s0, _, _ = _grad(net, opts, case, ppo, opts.shadow)
    g0 = net.grads_ext.clone()
    s1, _, _ = _grad(net, opts, case, ppo, opts.shadow)
    assert torch.equal(g0.view(torch.int32), net.grads_ext.view(torch.int32)) and torch.equal(s0.view(torch.int64), s1.view(torch.int64))


# ---------------------------------------------------------------------------------------------- 7. one optimiser step
@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_one_step_moves_the_actor_toward_the_teacher(opts):
    """A large constant coefficient, one gradient, one Adam step: the minibatch's MSE to the teacher falls; the same step without the
    term does not bring it down as far."""
    case = GC.case_of(opts)
    after = {}
    for name, coef in (("guided", 64.0), ("plain", 0.0)):
        net = G._net(opts)
        G._load(net, opts, case)
        ppo = G._ppo(opts, case)
        s0, _, _ = _grad(net, opts, case, ppo, opts.shadow, coef=coef)
        net.ppo_apply(ppo)
        s1, _, _ = _grad(net, opts, case, ppo, opts.shadow, coef=coef)
        assert torch.isfinite(net.params).all()
        after[name] = (float(s0[0]), float(s1[0]))
    print("MSE to the teacher before / after one step: guided %.5e -> %.5e, plain %.5e -> %.5e" % (after["guided"] + after["plain"]))
    assert after["guided"][0] == after["plain"][0]
    assert after["guided"][1] < after["guided"][0] and after["guided"][1] < after["plain"][1]


# ---------------------------------------------------------------------------------------------- 8. misuse
@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_misuse_is_refused(opts):
    import hgym
    case = GC.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    cols = [t.cuda().contiguous() for t in case["cols"]]
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    c = torch.ones(2, device="cuda")
    tmu = torch.zeros(case["S"] * cols[2].shape[1] + 4, device="cuda")
    idx = case["idx"].cuda()      # (held to the end: the batch descriptor carries its address, and a freed block is the next temporary's)
    batch = hgym.make_batch(*cols, idx)
    net.grads_ext.fill_(7.0)
    torch.cuda.synchronize()

    def good():
        return L.Guide(L.fptr(tmu), L.fptr(c), L.f64ptr(sums))

    def rc(gd, ppo=None):
        ppo = ppo or G._ppo(opts, case)
        return int(L.lib.hgym_ppo_grad_guide(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(batch), C.byref(gd), net.stream()))
    for field in ("teacher_mu", "coef", "sums"):
        gd = good()
        setattr(gd, field, None)
        assert rc(gd) == -1 and b"null" in L.lib.hgym_last_error(), field
    gd = good()
    gd.teacher_mu = C.cast(tmu.data_ptr() + 4, L.c_float_p)
    assert rc(gd) == -1 and b"16-byte" in L.lib.hgym_last_error()
    gd = good()
    gd.sums = C.cast(sums.data_ptr() + 4, L.c_f64_p)
    assert rc(gd) == -1
    assert rc(good(), ppo=G._ppo(opts, case, mirror_coef=0.5)) == -1 and b"mirror_coef" in L.lib.hgym_last_error()
    two = G._ppo(opts, case)
    two.world_size = 2
    assert rc(good(), ppo=two) == -1 and b"world_size" in L.lib.hgym_last_error()
    torch.cuda.synchronize()
    assert bool((net.grads_ext == 7.0).all()) and float(sums.sum()) == 0.0      # nothing was launched
    assert rc(good()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads_ext).all() and float(sums[1]) == 1.0 and float(sums[2]) == 0.0
