"""-m gpu: distillation on the device -- hgym_bc_grad against the float64 reference of tests/distill_common.py
on both paths, what it must leave zero, one optimiser step, the teacher's pass, guard bands, Distillation.update() on planted rows and
the runner on the task humanoid_distill.

Bars (the project's): the fp32 layer-by-layer path 1e-5 of the tensor's largest entry; the fused bf16 path per-tensor rel-L2 <= 5e-3
against the bf16-operand oracle (tests/test_fused_batch_edges_gpu.py).  BARS holds what a shape needs beyond that, with the measured value
and the reason; it is empty.

Where parameters AFTER a step are compared, the bound is bar * ||step|| + ||ulp/2||: the step is linear in the gradient there (the Adam
moments are planted so: v = the gradient's mean square, step count 1000 -- from zero moments the first step is lr * g / (|g| + eps), a sign
function that turns any error of a small gradient entry into a whole step), so the gradient's bar carries over to it, and half an fp32
ulp of each parameter is what storing the result in fp32 costs whatever the arithmetic."""
import copy
import os

import numpy as np
import pytest
import torch

import distill_common as D
import fused_batch_common as FB
import guard_common as G
from hgym import _lib as L
from oracle import ppo_oracle as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 1e-3
BARS = {}      # (net, B, loss_type): (bar, measured, reason)
_NETS = {}


# ------------------------------------------------------------------------------------------------ helpers
def _state_dict(name, views, std_key="std"):
    actor, critic = D.make_layers(name)
    sd = {std_key: torch.full((12,), 0.8 if std_key == "std" else float(np.log(0.8)))}
    for net, layers in (("actor", actor), ("critic", critic)):
        for l, (W, b) in enumerate(layers):
            sd["%s.%d.weight" % (net, 2 * l)], sd["%s.%d.bias" % (net, 2 * l)] = W, b
    assert list(sd) == list(views), (list(sd), list(views))
    return sd


def _cfg(name, std="scalar", max_batch=D.MAX_BATCH):
    from hgym import make_net_config
    prec, ad, cd = D.NETS[name]
    return make_net_config(ad[0], cd[0], ad[-1], ad[1:-1], cd[1:-1], prec, max_batch, noise_std_type=std, activation=D.activation(name),
                           fused_activation=name in D.TANH)


def _load(net, name, std="scalar"):
    for t in (net.adam_m, net.adam_v, net.grads_ext, net.opt_state):
        t.zero_()
    net.opt_state[L.OPT_LR] = LR
    net.load_state_dict(_state_dict(name, net.views, "log_std" if std == "log" else "std"))
    assert (net.shadow_ld(0) > 0) == (name in D.FUSED), "%s is not on the path this test is about" % name
    return net


def _net(name, std="scalar"):
    from hgym import NetBuffers
    if (name, std) not in _NETS:
        _NETS[name, std] = NetBuffers(_cfg(name, std), DEV, learning_rate=LR)
    return _load(_NETS[name, std], name, std)


def _inputs(net, case, shadow, alloc=None):
    """The device tensors of a case: obs, target, idx and, with `shadow`, the bf16 shadow of obs (selected rows rounded, pad columns zero,
    every other row NaN).  alloc: a guard_common allocator (Arena / Plain); None: plain torch."""
    put = (lambda t: t.to(DEV).contiguous()) if alloc is None else alloc.place
    dev = (lambda t: t) if alloc is None else (lambda t: t.to(DEV))
    obs, target, idx = put(dev(case["obs"])), put(dev(case["target"])), put(dev(case["idx"]))
    sh = None
    if shadow:
        s = torch.full((case["S"], net.shadow_ld(0)), float("nan"), dtype=torch.bfloat16)
        s[case["idx"]] = 0.0
        s[case["idx"], :case["obs"].shape[1]] = case["obs"][case["idx"]].to(torch.bfloat16)
        sh = put(dev(s))
    return obs, target, idx, sh


def _bc(net, tensors, loss_type, delta=1.0, sums=None):
    """One hgym_bc_grad on a NaN-filled gradient buffer -> (grads_ext, opt_state, sums) clones."""
    from hgym import make_bc_batch, make_bc_config
    obs, target, idx, sh = tensors
    sums = torch.zeros(2, dtype=torch.float64, device=DEV) if sums is None else sums
    net.grads_ext.fill_(float("nan"))
    net.bc_grad(make_bc_config(loss_type, delta), make_bc_batch(obs, idx, sh), target, sums)
    torch.cuda.synchronize()
    return net.grads_ext.clone(), net.opt_state.clone(), sums.clone()


def _actor_grads(net, grads_ext):
    base = net.params.data_ptr()
    return [grads_ext[(v.data_ptr() - base) // 4:][:v.numel()].view_as(v).cpu() for k, v in net.views.items() if k.startswith("actor.")]


def _check_grads(what, name, got, want, bar=None):
    bf16 = D.NETS[name][0] == "bf16"
    bar = (D.BF16_TOL if bf16 else D.F32_TOL) if bar is None else bar
    errs = [FB.rel_l2(g, w) if bf16 else D.rel_max(g, w) for g, w in zip(got, want)]
    print("%s: worst %s error %.3g (bar %.3g)" % (what, "rel-L2" if bf16 else "max / max", max(errs), bar))
    assert len(got) == len(want) and max(errs) <= bar, (what, errs)


def _half_ulp(w):
    a = w.float().abs()
    return ((torch.nextafter(a, torch.full_like(a, float("inf"))) - a) * 0.5).double()


# ------------------------------------------------------------------------------------------------ 1. gradient against float64
CASES = ([("g1", B, lt) for B in D.BATCHES for lt in D.LOSS_TYPES] + [("xbotl", 200, "mse")] +
         [("ragged", B, lt) for B in D.BATCHES for lt in D.LOSS_TYPES] +
         [("g1_tanh", 65, "mse"), ("g1_tanh", 200, "huber"), ("ragged_bf16", 65, "mse"), ("ragged_bf16", 200, "huber")])


@pytest.mark.parametrize("name, B, loss_type", CASES, ids=["%s-B%d-%s" % c for c in CASES])
def test_bc_grad_equals_the_float64_reference(name, B, loss_type):
    net, case = _net(name), D.make_case(name, B)
    want_loss, want = D.reference(name, case, loss_type)
    bf16 = D.NETS[name][0] == "bf16"
    bar = BARS.get((name, B, loss_type), (None,))[0]
    for shadow in ((False, True) if name in D.FUSED else (False,)):
        what = "%s B=%d %s %s" % (name, B, loss_type, "bf16 shadow" if shadow else "fp32 rows")
        tensors = _inputs(net, case, shadow)
        grads_ext, opt, sums = _bc(net, tensors, loss_type)
        assert torch.isfinite(grads_ext).all(), what
        _check_grads(what, name, _actor_grads(net, grads_ext), want, bar)
        assert float(sums[1]) == 1.0
        np.testing.assert_allclose(float(sums[0]), want_loss, rtol=D.BF16_TOL if bf16 else D.F32_TOL, err_msg=what)
        sq = sum(float((g.double() ** 2).sum()) for g in _actor_grads(net, grads_ext))
        np.testing.assert_allclose(float(opt[L.OPT_GRAD_SQNORM]), sq, rtol=1e-6, atol=2e-11, err_msg=what)


# ------------------------------------------------------------------------------------------------ 2. what must be zero is zero
@pytest.mark.parametrize("name, std", [("g1", "scalar"), ("g1", "log"), ("ragged", "scalar")])
def test_what_is_not_trained_stays_exactly_as_it_is(name, std):
    from hgym import make_ppo_config
    net, case = _net(name, std), D.make_case(name, 65)
    A, P_ = 12, net.P
    critic_off = net.bucket_split
    net.opt_state[L.OPT_KL_SUM:L.OPT_AUX_SUM + 1] = torch.arange(1, 10, dtype=torch.float64, device=DEV) * 0.37      # anything: it must survive
    net.opt_state[L.OPT_GRAD_NORM] = 0.0
    before = dict(params=net.params.clone(), sigma=net.sigma.clone(), opt=net.opt_state.clone())
    want_loss, _ = D.reference(name, case, "huber")
    grads_ext, opt, sums = _bc(net, _inputs(net, case, False), "huber")
    bits = grads_ext.view(torch.int32)
    assert int(bits[:A].abs().max()) == 0 and int(bits[critic_off:P_ + 1].abs().max()) == 0, "std / critic / KL slot are not +0.0"
    assert int((bits[A:critic_off] != 0).sum()) > 0.9 * (critic_off - A)
    keep = [i for i in range(L.OPT_STATE) if i != L.OPT_GRAD_SQNORM]
    assert torch.equal(opt[keep], before["opt"][keep]), (opt, before["opt"])
    assert float(sums[1]) == 1.0 and abs(float(sums[0]) - want_loss) <= 5e-3 * want_loss
    net.ppo_apply(make_ppo_config(max_grad_norm=3.0e38, desired_kl=0.0, adaptive=False, grad_norm_ready=False))
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(net.params[:A], before["params"][:A]) and same(net.sigma, before["sigma"]), "sigma moved"
    assert same(net.params[critic_off:], before["params"][critic_off:]), "a critic parameter moved"
    assert not same(net.params[A:critic_off], before["params"][A:critic_off])
    assert int(net.adam_m[critic_off:].view(torch.int32).abs().max()) == 0 and int(net.adam_v[:A].view(torch.int32).abs().max()) == 0
    o = net.opt_state
    assert float(o[L.OPT_LR]) == LR and float(o[L.OPT_STEP]) == 1.0
    sums_slots = [L.OPT_KL_SUM, L.OPT_SURROGATE_SUM, L.OPT_VALUE_SUM, L.OPT_ENTROPY_SUM, L.OPT_MINIBATCHES, L.OPT_KL_LAST, L.OPT_AUX_SUM]
    assert torch.equal(o[sums_slots], before["opt"][sums_slots])


# ------------------------------------------------------------------------------------------------ 3. one optimiser step
def _planted_moments(net, want, step=1000.0):
    """v = the reference gradient's mean square over the actor, m = 0, `step` steps done: Adam's step is then linear in the gradient to
    1e-3 of it wherever g^2 < v, and far larger than an fp32 ulp of the parameters (module docstring)."""
    c2 = float(sum((g ** 2).sum() for g in want) / sum(g.numel() for g in want))
    net.adam_m.zero_()
    net.adam_v.fill_(c2)
    net.opt_state[L.OPT_STEP] = step
    return c2


@pytest.mark.parametrize("name, loss_type", [("g1", "mse"), ("g1", "huber"), ("ragged", "mse")])
def test_one_step_equals_float64_adam_on_the_reference_gradient(name, loss_type):
    from hgym import make_ppo_config
    net, case = _net(name), D.make_case(name, 200)
    _, want = D.reference(name, case, loss_type)
    c2 = _planted_moments(net, want)
    actor = [t.double() for wb in D.make_layers(name)[0] for t in wb]
    opt = D.Adam64(actor)
    opt.v, opt.t = [torch.full_like(t, c2) for t in actor], 1000
    ref = opt.step(actor, want, LR)
    _bc(net, _inputs(net, case, False), loss_type)
    net.ppo_apply(make_ppo_config(max_grad_norm=3.0e38, desired_kl=0.0, adaptive=False, grad_norm_ready=False))
    torch.cuda.synchronize()
    bar = D.BF16_TOL if D.NETS[name][0] == "bf16" else D.F32_TOL
    got = [v.detach().cpu().double() for k, v in net.views.items() if k.startswith("actor.")]
    for k, (g, r, w0) in enumerate(zip(got, ref, actor)):
        err, step = float((g - r).norm()), float((r - w0).norm())
        bound = bar * step + float(_half_ulp(r).norm())
        print("%s %s tensor %d: |error| %.3g, bound %.3g (step %.3g)" % (name, loss_type, k, err, bound, step))
        assert step > 0 and err <= bound, (name, loss_type, k, err, bound)
    # the operand copies are current: a forward now equals a forward after a full refresh
    x = torch.randn(70, D.NETS[name][1][0], generator=torch.Generator().manual_seed(5)).to(DEV)
    y1 = net.forward(0, x).clone()
    net.sync_shadow()
    y2 = net.forward(0, x)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)) and torch.isfinite(y1).all()


@pytest.mark.parametrize("name", ["g1", "ragged"])
def test_first_step_from_zero_moments(name):
    """The first real step of a run: m = v = 0, so the step is lr * g / (|g| + eps) -- the gradient's sign, whatever its size.  Held on the
    entries a gradient error cannot flip: the bar admits a per-tensor error of bar * ||g||_2 =: tau (all of it in one entry at worst), so
    an entry with |g_ref| >= 2 tau has the reference's sign on the device and |g_dev| >= tau there, and its step lies in
    lr * [1 - eps / tau, 1]; on top come the fp32 arithmetic of the step (a handful of roundings, 1e-6 of it) and half an ulp of the stored
    parameter.  At least a twentieth of every tensor's entries must qualify, or the case says nothing (the widest tensor, 256 x 141, has
    2 tau = 1.9 rms of its entries: 5.7 % of a Gaussian, 5.9 % of the reference gradient)."""
    from hgym import make_ppo_config
    net, case = _net(name), D.make_case(name, 200)
    _, want = D.reference(name, case, "mse")
    actor = [t.double() for wb in D.make_layers(name)[0] for t in wb]
    ref = D.Adam64(actor).step(actor, want, LR)
    _bc(net, _inputs(net, case, False), "mse")
    net.ppo_apply(make_ppo_config(max_grad_norm=3.0e38, desired_kl=0.0, adaptive=False, grad_norm_ready=False))
    torch.cuda.synchronize()
    assert float(net.opt_state[L.OPT_STEP]) == 1.0
    bar = D.BF16_TOL if D.NETS[name][0] == "bf16" else D.F32_TOL
    got = [v.detach().cpu().double() for k, v in net.views.items() if k.startswith("actor.")]
    for k, (w1, r, w0, g) in enumerate(zip(got, ref, actor, want)):
        tau = bar * float(g.norm())
        sel = g.abs() >= 2 * tau
        share = float(sel.double().mean())
        bound = LR * (1e-8 / tau + 1e-6) + _half_ulp(r)
        err = (w1 - r).abs()
        print("%s tensor %d: %.0f %% of the entries held, worst error / bound %.3g" % (name, k, 100 * share, float((err / bound)[sel].max())))
        assert share >= 0.05 and bool((err <= bound)[sel].all()), (name, k, share)
        assert bool(((w1 - w0).abs() <= LR * (1 + 1e-6) + 2 * _half_ulp(r)).all())      # and no entry anywhere moves by more than lr


@pytest.mark.parametrize("name", ["xbotl", "ragged"])
def test_an_auxiliary_heads_region_is_left_zero(name):
    """The library's statement for a net WITH an auxiliary head (the Python layer refuses one): its region of the gradient vector, like
    std's, the critic's and the KL slot, is +0.0 after hgym_bc_grad on a NaN-filled buffer, on the fused layout and on the layer-by-layer one."""
    from hgym import NetBuffers, make_net_config
    prec, ad, cd = D.NETS[name]
    aux = dict(aux_hidden=[512, 256, 256], aux_out=73, aux_target_offset=219 - 73) if name == "xbotl" else \
        dict(aux_hidden=[16, 8], aux_out=5, aux_target_offset=3)
    net = NetBuffers(make_net_config(ad[0], cd[0], ad[-1], ad[1:-1], cd[1:-1], prec, D.MAX_BATCH, **aux), DEV, learning_rate=LR)
    assert any(k.startswith("denoiser.") for k in net.views) and (net.shadow_ld(0) > 0) == (name in D.FUSED)
    g = torch.Generator().manual_seed(9)
    net.params.copy_((torch.randn(net.P, generator=g) * 0.05).to(DEV))
    net.params[:12] = 0.8
    net.sync_shadow()
    case = D.make_case(name, 65)
    grads_ext, opt, sums = _bc(net, _inputs(net, case, False), "mse")
    bits, A, critic_off = grads_ext.view(torch.int32), 12, net.bucket_split
    aux_off = int(L.lib.hgym_net_param_offset(__import__("ctypes").byref(net.cfg), 2))
    assert critic_off < aux_off < net.P
    assert int(bits[:A].abs().max()) == 0 and int(bits[critic_off:].abs().max()) == 0, "std / critic / auxiliary head / KL slot are not +0.0"
    assert torch.isfinite(grads_ext).all() and int((bits[A:critic_off] != 0).sum()) > 0.9 * (critic_off - A) and float(sums[1]) == 1.0


# ------------------------------------------------------------------------------------------------ the algorithm object, shared
OBS, PRIV, ACT = 141, 219, 12


def _alg(N=64, T=8, G_=4, epochs=2, lr=LR, loss_type="mse", teacher_max_batch=None):
    """A Distillation over a StudentTeacher of the smallest fused widths, student = make_layers("g1", 11), teacher = ("g1", 21)."""
    from humanoid.algo import Distillation, PPO, StudentTeacher
    PPO.precision = "bf16"
    pol = StudentTeacher(OBS, PRIV, ACT, student_hidden_dims=[256, 128, 128], teacher_hidden_dims=[256, 128, 128],
                         critic_hidden_dims=[256, 128, 128])
    pol.teacher_max_batch = teacher_max_batch
    alg = Distillation(pol, num_learning_epochs=epochs, gradient_length=G_, learning_rate=lr, loss_type=loss_type, device="cuda:0")
    alg.init_storage(N, T, [OBS], [PRIV], [ACT])
    sd = _state_dict("g1", alg.net.views)
    sd["std"] = torch.full((12,), 0.1)
    alg.net.load_state_dict(sd)
    teacher = {"actor.%d.%s" % (2 * l, k): t for l, wb in enumerate(D.make_layers("g1", 21)[0]) for k, t in zip(("weight", "bias"), wb)}
    assert pol.load_state_dict(dict(teacher, std=torch.ones(12))) is False and pol.loaded_teacher
    return alg


def _plant_rows(alg, seed=7):
    st = alg.storage
    T, N = st.num_transitions_per_env, st.num_envs
    obs = torch.randn(T * N, OBS, generator=torch.Generator().manual_seed(seed))
    st._obs_all[:T].copy_(obs.view(T, N, OBS).to(DEV))
    st.shadow_valid = [False] * T      # rows written by hand: no policy launch left their bf16 shadow
    return obs


# ------------------------------------------------------------------------------------------------ 4. the teacher's pass
def test_teacher_pass_in_ragged_pieces():
    """T N = 512 rows through a teacher net of max_batch 200: pieces of 192, 192 and 128 rows."""
    alg = _alg(teacher_max_batch=200)
    pol, st = alg.actor_critic, alg.storage
    assert int(pol._teacher_net.cfg.max_batch) == 200 and pol._teacher_net.shadow_ld(0) > 0      # the fused path, placeholder critic and all
    obs = _plant_rows(alg)
    st.teacher_actions.fill_(float("nan"))
    before = alg._deferred_ready, st.values.clone()
    alg.compute_returns(None)
    torch.cuda.synchronize()
    got = st.teacher_actions.flatten(0, 1).cpu()
    assert torch.equal(st.values, before[1]) and float(st.returns.abs().max()) == 0.0      # no GAE, no critic
    want = P.mlp_forward(obs.double(), FB.dbl(D.make_layers("g1", 21)[0]))
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print("teacher pass: max error %.3g of the activation scale %.3g" % (err / scale, scale))
    assert torch.isfinite(got).all() and err <= 1e-2 * scale
    slots = torch.cat([pol.teacher_inference(st._obs_all[t]) for t in range(st.num_transitions_per_env)]).cpu()
    assert torch.equal(got.view(torch.int32), slots.view(torch.int32)), "the pass in pieces differs from hgym_mlp_forward slot by slot"


# ------------------------------------------------------------------------------------------------ 5. guard bands
@pytest.mark.parametrize("name, shadow", [("g1", False), ("g1", True), ("ragged", False)])
def test_bc_grad_stays_inside_the_callers_buffers(name, shadow):
    from hgym import NetBuffers
    case = D.make_case(name, 65)
    cfg = _cfg(name)
    out = {}
    for side in ("twin", "guarded"):
        if side == "twin":
            alloc, arenas = G.Plain(DEV), ()
            net = NetBuffers(cfg, DEV, learning_rate=LR)
        else:
            na = G.Arena(DEV, G.net_arena_bytes(cfg))
            net = G.guard_net(cfg, na, learning_rate=LR)
            ld = max(net.shadow_ld(0), 1)
            alloc = G.Arena(DEV, G.arena_bytes(case["obs"].numel() * 4, case["target"].numel() * 4, case["B"] * 8, case["S"] * ld * 2, 16))
            arenas = (na, alloc)
        _load(net, name)
        tensors = _inputs(net, case, shadow, alloc)
        sums = alloc.zeros(2, torch.float64)
        grads_ext, opt, s = _bc(net, tensors, "huber", sums=sums)
        torch.cuda.synchronize()
        for a in arenas:
            a.verify("hgym_bc_grad %s B=65 %s" % (name, "bf16 shadow" if shadow else "fp32 rows"))
        out[side] = (grads_ext, opt, s)
    for a, b in zip(out["twin"], out["guarded"]):
        assert torch.isfinite(b).all()
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "the guarded run differs from its twin"


# ------------------------------------------------------------------------------------------------ 6. the algorithm on planted storage
def _restate(alg, obs, lr, updates=1, opt=None, layers=None):
    """distill_common.distill_update on the rows in the storage (bf16-operand model), the targets the device's own teacher pass."""
    st = alg.storage
    layers = FB.dbl(D.make_layers("g1", 11)[0]) if layers is None else layers
    target = st.teacher_actions.flatten(0, 1).cpu().double()
    seq = []
    for _ in range(updates):
        layers, losses, opt = D.distill_update(layers, obs.double(), target, st.num_envs, alg.gradient_length, alg.num_learning_epochs, lr,
                                               alg.loss_type, alg.huber_delta, opt=opt, quant=D.q64)
        seq.append(sum(losses) / len(losses))
    return layers, seq, opt


def test_update_equals_the_float64_restatement_of_its_four_steps():
    alg = _alg()
    obs = _plant_rows(alg)
    alg.compute_returns(None)
    torch.cuda.synchronize()
    # planted moments (module docstring): v from the first slice's reference gradient
    student = FB.dbl(D.make_layers("g1", 11)[0])
    target = alg.storage.teacher_actions.flatten(0, 1).cpu().double()
    _, g0 = D.bc_loss_and_grads(student, obs[:256].double(), target[:256], quant=D.q64)
    c2 = _planted_moments(alg.net, D.flat(g0))
    w0 = D.flat(student)
    opt = D.Adam64(w0)
    opt.v, opt.t = [torch.full_like(t, c2) for t in w0], 1000
    draws = alg._perm_draws, int(alg._perm_draws_dev)
    # the restatement, step by step: the bound needs every step's length
    mb, tensors, steps, losses = 4 * 64, w0, [0.0] * len(w0), []
    for _ in range(2):
        for k in range(2):
            cur = [(tensors[2 * i], tensors[2 * i + 1]) for i in range(4)]
            loss, grads = D.bc_loss_and_grads(cur, obs[k * mb:(k + 1) * mb].double(), target[k * mb:(k + 1) * mb], quant=D.q64)
            new = opt.step(tensors, D.flat(grads), LR)
            steps = [s + float((n - t).norm()) for s, n, t in zip(steps, new, tensors)]
            tensors = new
            losses.append(float(loss))
    value_loss, behavior = alg.update()
    torch.cuda.synchronize()
    assert value_loss == 0.0 and behavior == alg.last_behavior_loss
    np.testing.assert_allclose(behavior, sum(losses) / 4, rtol=D.BF16_TOL)
    assert float(alg.net.opt_state[L.OPT_STEP]) == 1004.0 and float(alg.net.opt_state[L.OPT_LR]) == LR
    assert (alg._perm_draws, int(alg._perm_draws_dev)) == draws and alg.storage.step == 0      # no permutation was drawn
    got = [v.detach().cpu().double() for k, v in alg.net.views.items() if k.startswith("actor.")]
    for k, (g, r, s) in enumerate(zip(got, tensors, steps)):
        err, bound = float((g - r).norm()), D.BF16_TOL * s + 4 * float(_half_ulp(r).norm())
        print("update, tensor %d: |error| %.3g, bound %.3g" % (k, err, bound))
        assert err <= bound, (k, err, bound)


def test_ten_updates_on_the_same_rows_lower_the_loss_every_time():
    """The float64 restatement of this run (lr 1e-3, these seeds, bf16-operand model, run on the CPU when the test was written) falls
    0.01238, 0.00389, 0.00212, 0.00141, 0.00096, 0.00068, 0.00052, 0.00042, 0.00036, 0.00031: every step down, a factor 39.7 over the ten."""
    alg = _alg()
    obs = _plant_rows(alg)
    seq = []
    for _ in range(10):
        alg.storage._obs_all[:8].copy_(obs.view(8, 64, OBS).to(DEV))      # update() rotated slot T into slot 0: the rows stay fixed
        alg.storage.shadow_valid = [False] * 8
        alg.compute_returns(None)
        seq.append(alg.update()[1])
    print("behaviour loss over ten updates:", ["%.5f" % s for s in seq])
    assert all(np.isfinite(seq)) and all(b < a for a, b in zip(seq, seq[1:])), seq


# ------------------------------------------------------------------------------------------------ 7. the runner
def _cfgs(task, num_envs, seed):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=" + task, "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=task))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4
    train_cfg.runner.num_steps_per_env = 8
    return args, env_cfg, train_cfg


def _runner(task, log_root, seed=31, exact=False, precision="bf16", actor_hidden_dims=None, student_hidden_dims=None, **alg_kw):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    PPO.precision = precision
    args, env_cfg, train_cfg = _cfgs(task, 64, seed)
    if actor_hidden_dims is not None:
        train_cfg.policy.actor_hidden_dims = list(actor_hidden_dims)
    if student_hidden_dims is not None:
        train_cfg.policy.student_hidden_dims = list(student_hidden_dims)
    if task == "humanoid_distill":
        train_cfg.algorithm.gradient_length = 4
    for k, v in alg_kw.items():
        setattr(train_cfg.algorithm, k, v)
    train_cfg.runner.save_interval = 100
    if exact:
        train_cfg.runner.exact_resume = True
    env, _ = task_registry.make_env(name=task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None if log_root is None else str(log_root))
    return runner


class _Scalars:
    def __init__(self):
        self.tags = {}

    def add_scalar(self, tag, value, it):
        self.tags.setdefault(tag, []).append(float(value))


@pytest.fixture(scope="module")
def teacher_ckpt(tmp_path_factory):
    """A random-weight teacher, saved through a PPO runner's save()."""
    torch.manual_seed(3)
    r = _runner("humanoid_ppo", None)
    path = str(tmp_path_factory.mktemp("teacher") / "model_0.pt")
    r.save(path)
    r.wait_for_saves()
    return path, {k: v.detach().cpu().clone() for k, v in r.alg.actor_critic.state_dict().items()}


def _frozen(runner):
    net = runner.alg.net
    return net.params[:12].clone(), net.sigma.clone(), net.params[net.bucket_split:].clone()


@pytest.fixture(autouse=True)
def _bf16_afterwards():
    yield
    from humanoid.algo import PPO
    PPO.precision = "bf16"


WIDE = [512, 128, 128]      # a student whose first width is one the one-launch rollout step is instantiated for
# (student widths, HGYM_FUSE_ROLLOUT, HGYM_ROLLOUT_CRITIC, precision) -> the loop plan's `fuse`
PLANS = [(WIDE, "1", "auto", "bf16", "inline"), (WIDE, "1", "deferred", "bf16", "deferred"), (WIDE, "0", "auto", "bf16", None),
         (None, "1", "auto", "bf16", None), (None, "0", "auto", "f32", None)]


@pytest.mark.parametrize("student, fuse, critic, precision, plan", PLANS,
                         ids=["wide-inline", "wide-deferred", "wide-stepwise", "task-student-stepwise", "task-student-f32"])
def test_runner_distils_on_every_rollout_form(teacher_ckpt, tmp_path, monkeypatch, student, fuse, critic, precision, plan):
    """load(teacher) then learn(3) under every loop plan a distillation run can get, the plan asserted: the one-launch rollout with the
    critic's tiles inline and with the critic deferred behind it (a student of first width 512; deferred_values() runs in the rollout,
    compute_returns must not be thrown by it), the stepwise rollout with HGYM_FUSE_ROLLOUT=0, the stepwise rollout the task's own student
    gets whatever the knob says (first width 256: no one-launch step exists for it), and fp32 (the layer-by-layer path, where the device's
    forward is the module's own arithmetic: there also the exported JIT policy against act_inference to 1e-5)."""
    from humanoid.algo import Distillation, StudentTeacher
    from humanoid.algo.ppo.on_policy_runner import _plan_loop
    monkeypatch.setenv("HGYM_FUSE_ROLLOUT", fuse)
    monkeypatch.setenv("HGYM_ROLLOUT_CRITIC", critic)
    path, teacher_sd = teacher_ckpt
    r = _runner("humanoid_distill", tmp_path, precision=precision, student_hidden_dims=student)
    assert isinstance(r.alg, Distillation) and isinstance(r.alg.actor_critic, StudentTeacher) and r.alg.net.cfg.max_batch == 4 * 64
    assert (r.alg.net.shadow_ld(0) > 0) == (precision == "bf16")
    assert _plan_loop(r.env, r.alg, r.device, True).fuse == plan
    with pytest.raises(RuntimeError, match="teacher not loaded"):
        r.learn(num_learning_iterations=1)
    r.load(path)
    assert r.current_learning_iteration == 0 and r.alg.actor_critic.loaded_teacher and float(r.alg.net.opt_state[L.OPT_STEP]) == 0.0
    for k, v in r.alg.actor_critic.teacher.state_dict().items():
        assert torch.equal(v.cpu(), teacher_sd["actor." + k]), k
    frozen, student0 = _frozen(r), r.alg.net.params[12:r.alg.net.bucket_split].clone()
    r.writer = rec = _Scalars()      # (in place of the tensorboard writer, which would otherwise also create the directory)
    os.makedirs(r.log_dir, exist_ok=True)
    r.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    r.wait_for_saves()
    torch.cuda.synchronize()
    assert len(rec.tags["Loss/behavior"]) == 3 and all(np.isfinite(rec.tags["Loss/behavior"])) and min(rec.tags["Loss/behavior"]) > 0.0
    assert set(rec.tags["Loss/surrogate"]) == {0.0} and set(rec.tags["Loss/value_function"]) == {0.0}      # a cloning run has neither
    if plan == "deferred":      # the critic ran behind the rollout, and compute_returns used its result up
        assert r.alg.storage.time_outs is not None and not r.alg._deferred_ready
    assert float(r.alg.net.opt_state[L.OPT_STEP]) == 3 * 2 and r.current_learning_iteration == 3
    for a, b in zip(frozen, _frozen(r)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the critic or sigma moved"
    assert not torch.equal(student0, r.alg.net.params[12:r.alg.net.bucket_split]) and torch.isfinite(r.alg.net.params).all()
    ck = torch.load(os.path.join(r.log_dir, "model_3.pt"), map_location="cpu")
    assert list(ck["model_state_dict"]) == list(r.alg.actor_critic.state_dict()) and "teacher.6.bias" in ck["model_state_dict"]
    if precision == "f32":      # the exported policy is the student
        from humanoid.utils import export_policy_as_jit
        export_policy_as_jit(r.alg.actor_critic, str(tmp_path / "exported"))
        jit = torch.jit.load(str(tmp_path / "exported" / "policy_1.pt"))
        x = torch.randn(33, r.env.num_obs, generator=torch.Generator().manual_seed(2))
        with torch.no_grad():
            want = r.alg.actor_critic.act_inference(x.to(DEV)).cpu()
            got = jit(x)
        assert float((got - want).abs().max()) <= 1e-5
    if plan == "inline":        # the student's half of the checkpoint trains on under PPO
        p = _runner("humanoid_ppo", None, seed=32, actor_hidden_dims=WIDE)
        p.alg.actor_critic.load_state_dict(r.alg.actor_critic.student_state_dict(), strict=True)
        before = p.alg.net.params.clone()
        assert torch.equal(before[12:p.alg.net.bucket_split], r.alg.net.params[12:r.alg.net.bucket_split])
        p.learn(num_learning_iterations=1, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        assert torch.isfinite(p.alg.net.params).all() and not torch.equal(before, p.alg.net.params)


def test_resumed_distillation_is_the_uninterrupted_one(teacher_ckpt, tmp_path):
    """learn(3), save, a new runner, load, learn(2) against learn(5): bit for bit -- one rank, the device permutation plays no part, the
    env's state travels in the sidecar (runner.exact_resume), every sum of the update is formed in a fixed order."""
    path, _ = teacher_ckpt
    u = _runner("humanoid_distill", tmp_path / "u", exact=True)
    u.load(path)
    u.learn(num_learning_iterations=5, init_at_random_ep_len=True)
    a = _runner("humanoid_distill", tmp_path / "a", exact=True)
    a.load(path)
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    a.wait_for_saves()
    b = _runner("humanoid_distill", tmp_path / "b", exact=True)      # (the same seed: the exploration noise's key is the run's seed)
    b.load(os.path.join(a.log_dir, "model_3.pt"))
    assert b.current_learning_iteration == 3 and b.alg.actor_critic.loaded_teacher and float(b.alg.net.opt_state[L.OPT_STEP]) == 6.0
    b.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    for name in ("params", "adam_m", "adam_v"):
        x, y = getattr(u.alg.net, name), getattr(b.alg.net, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s differs in %d places" % (name, int((x != y).sum()))
    assert float(b.alg.net.opt_state[L.OPT_STEP]) == 10.0 and b.current_learning_iteration == 5
