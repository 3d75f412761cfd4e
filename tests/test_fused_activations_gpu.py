"""-m gpu: HgymNetConfig.fused_activation -- the fused bf16 forward and update kernels (hgym_fused.hpp: the GA instantiations) under
every supported activation, against the float64 restatement tests/test_activations_gpu.py uses for the layer-by-layer path
(layer_path_common.restated with quant = bf16 rounding: operands and every hidden y rounded where the kernels round, the derivative
taken from the ROUNDED y).  The bars are that file's: forward rel-L2 2e-3, worst output / output scale 5e-3 (2e-2 under sigmoid, for the
reason given there), gradient 5e-3 per tensor, critic.6.bias against ||d_val||.

The one-launch rollout / evaluation step (hgym_rollout_step, hgym_rollout_eval_step: rollout_step_act_kernel) is compared bit for bit
with PPO.act / act_inference + the env step on the same flag-on net."""
import math
import os
import numpy as np
import pytest
import torch
import torch.nn as nn

import bf16_report as BR
import layer_path_common as LP
from oracle import ppo_oracle as P
from hgym import _lib as L

pytestmark = pytest.mark.gpu

ACTS = {
    "elu0.5": nn.ELU(alpha=0.5),
    "selu": nn.SELU(),
    "relu": nn.ReLU(),
    "leaky0.01": nn.LeakyReLU(0.01),
    "tanh": nn.Tanh(),
    "sigmoid": nn.Sigmoid(),
}
FWD_TOL, FWD_MAX_TOL, SIGMOID_FWD_MAX_TOL, GRAD_TOL = 2e-3, 5e-3, 2e-2, 5e-3      # tests/test_activations_gpu.py
SHAPES = {
    "xbotl": ([512, 256, 128], [768, 256, 128]),
    "256x3": ([256, 256, 256], [256, 256, 256]),
    "big_actor": ([768, 256, 128], [768, 256, 128]),     # refused by the fused tiles at any activation
}


def _q64(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _dbl(layers):
    return [(W.double(), b.double()) for W, b in layers]


def _rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _split(net, flat):
    base = net.params.data_ptr()
    return [flat[(v.data_ptr() - base) // 4:][:v.numel()].view_as(v) for v in net.views.values()]


def _setup(act, shape, max_batch, seed, precision="bf16", fused_activation=True, **kw):
    from hgym import NetBuffers, make_net_config
    ah, ch = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    p = P.Params.random(705, 219, 12, ah, ch, g)
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    net = NetBuffers(make_net_config(705, 219, 12, ah, ch, precision, max_batch, activation=act, fused_activation=fused_activation, **kw),
                     "cuda", learning_rate=1e-3)
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    return p, net, g


# ---------------------------------------------------------------------------------------------- 1. path selection
@pytest.mark.parametrize("name", list(ACTS))
def test_path_selection(name, monkeypatch):
    act = ACTS[name]
    for shape, ld in (("xbotl", (768, 256)), ("256x3", (768, 256))):
        _, on, _ = _setup(act, shape, 64, 1)
        _, off, _ = _setup(act, shape, 64, 1, fused_activation=False)
        assert (on.shadow_ld(0), on.shadow_ld(1)) == ld and off.shadow_ld(0) == 0 and off.shadow_ld(1) == 0
    assert _setup(act, "big_actor", 64, 1)[1].shadow_ld(0) == 0
    assert _setup(act, "xbotl", 64, 1, precision="f32")[1].shadow_ld(0) == 0
    monkeypatch.setenv("HGYM_NO_FUSED", "1")
    assert _setup(act, "xbotl", 64, 1)[1].shadow_ld(0) == 0


# ---------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("shape", ["xbotl", "256x3"])
@pytest.mark.parametrize("name", list(ACTS))
def test_forward_vs_restated_reference(name, shape):
    """hgym_mlp_forward of the actor and the critic and the inference policy, M in {1, 33, 65, 200} of max_batch = 200: off the 32- and
    64-row tile edges, one tile and several."""
    from humanoid.algo.ppo.actor_critic import ActorCritic
    act = ACTS[name]
    M = 200
    p, net, g = _setup(act, shape, M, 21)
    assert net.shadow_ld(0) > 0
    fwd, _ = LP.restated(act)
    obs = (torch.randn(M, 705, generator=g) * 2).clamp(-18, 18)
    priv = (torch.randn(M, 219, generator=g) * 2).clamp(-18, 18)
    with torch.no_grad():
        ref = {0: fwd(obs.double(), _dbl(p.actor), quant=_q64), 1: fwd(priv.double(), _dbl(p.critic), quant=_q64)}
    xs = {0: obs.cuda(), 1: priv.cuda()}
    ah, ch = SHAPES[shape]
    ac = ActorCritic(705, 219, 12, actor_hidden_dims=ah, critic_hidden_dims=ch, activation=act, fused_activation=True)
    ac.load_state_dict(dict(zip(list(net.views), p.tensors())))
    ac.bind(net)
    tol_max = SIGMOID_FWD_MAX_TOL if name == "sigmoid" else FWD_MAX_TOL
    for m in (1, 33, 65, M):
        outs = [("actor", 0, net.forward(0, xs[0][:m].contiguous())), ("critic", 1, net.forward(1, xs[1][:m].contiguous())),
                ("act_inference", 0, ac.act_inference(xs[0][:m]))]
        torch.cuda.synchronize()
        for what, which, y in outs:
            assert torch.isfinite(y).all()
            d, r = y.cpu().double() - ref[which][:m], ref[which][:m]
            what = "fused forward %s %s %s, M = %d vs restated reference" % (name, shape, what, m)
            BR.check(what + ", rel-L2", float(d.norm() / r.norm()), FWD_TOL)
            BR.check(what + ", worst output", float(d.abs().max() / ref[which].abs().max()), tol_max)


# ---------------------------------------------------------------------------------------------- 3. planted pre-activations
PLANTED = [0.0, 1e-6, -1e-6, 2.0 ** -9, -2.0 ** -9, 0.5, -0.5, 3.0, -3.0, 18.0, -18.0, 90.0, -90.0]


@pytest.mark.parametrize("name", list(ACTS))
def test_planted_preactivations(name):
    """First-layer weights zero, its 512 biases cycling through PLANTED: every first hidden y is f(bias).  The first hidden activations are
    not reachable from Python (they live in the caller-opaque workspace), so they are observed through the outputs, at the forward bars,
    with M off the tile sizes; everything finite, also at |z| = 90 where exp2 gives 0 or inf.  Then one gradient: finite, and the
    first-layer gradient rows of the units whose f' is exactly 0 on the rounded y (ReLU at z <= 0, Tanh at +-1, Sigmoid at 1) exactly 0,
    as the reference gives by the same rule."""
    from hgym import make_ppo_config, make_batch
    act = ACTS[name]
    S, B = 200, 161
    p, net, g = _setup(act, "xbotl", S, 31)
    bias = torch.tensor([PLANTED[i % len(PLANTED)] for i in range(512)])
    p.actor[0] = (torch.zeros_like(p.actor[0][0]), bias)
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    fwd, bwd = LP.restated(act)
    f, df = LP.act_fns(act)
    obs, priv = torch.randn(S, 705, generator=g), torch.randn(S, 219, generator=g)
    with torch.no_grad():
        ref = fwd(obs.double(), _dbl(p.actor), quant=_q64)
    y = net.forward(0, obs.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    d = y.cpu().double() - ref
    BR.check("planted %s: outputs vs restated reference, rel-L2" % name, float(d.norm() / ref.norm()), FWD_TOL)
    BR.check("planted %s: worst output" % name, float(d.abs().max() / ref.abs().max()), SIGMOID_FWD_MAX_TOL if name == "sigmoid" else FWD_MAX_TOL)
    actions, mu_o = torch.randn(S, 12, generator=g), torch.randn(S, 12, generator=g) * 0.3
    sg_o = torch.rand(S, 12, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    lp_o = P.gaussian_log_prob(actions, ref.float(), ref.float() * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    cols = (obs, priv, actions, val, adv, ret, lp_o, mu_o, sg_o)
    net.ppo_grad(make_ppo_config(), make_batch(*[t.cuda().contiguous() for t in cols], idx.cuda()))
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads).all()
    gv = net.grad_views()
    dead = df(_q64(f(bias.double()))) == 0
    if name in ("relu", "tanh", "sigmoid"):
        assert int(dead.sum()) > 0
    assert (gv["actor.0.weight"][dead.cuda()] == 0).all() and (gv["actor.0.bias"][dead.cuda()] == 0).all()
    assert (gv["actor.0.bias"][~dead.cuda()] != 0).any()


# ---------------------------------------------------------------------------------------------- 4. gradient
GRAD_CASES = [(a, "xbotl", xb, False) for a in ACTS for xb in (False, True)] + \
             [(a, "256x3", xb, False) for a in ("tanh", "relu") for xb in (False, True)] + [("tanh", "xbotl", True, True)]


@pytest.mark.parametrize("name,shape,xb16,unclipped", GRAD_CASES, ids=["%s-%s-%s%s" % (a, s, "shadow" if x else "fp32rows", "-vu" if u else "")
                                                                       for a, s, x, u in GRAD_CASES])
def test_gradient_vs_restated_reference(name, shape, xb16, unclipped, monkeypatch):
    """hgym_ppo_grad on one minibatch (S = 5000 stored rows, B = 4096: 64 tiles) against the oracle's PPO loss and backward with the
    restated MLP, per parameter tensor; input rows gathered from the fp32 storage or from bf16 shadows."""
    from hgym import make_ppo_config, make_batch
    act = ACTS[name]
    S, B = 5000, 4096
    p, net, g = _setup(act, shape, B, 12)
    assert net.shadow_ld(0) > 0
    fwd, bwd = LP.restated(act)
    monkeypatch.setattr(P, "mlp_forward", fwd)
    monkeypatch.setattr(P, "mlp_backward", bwd)
    obs, priv = torch.randn(S, 705, generator=g), torch.randn(S, 219, generator=g)
    actions, mu_o = torch.randn(S, 12, generator=g), torch.randn(S, 12, generator=g) * 0.3
    sg_o = torch.rand(S, 12, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    with torch.no_grad():
        mu_now = fwd(obs, p.actor)
    lp_o = P.gaussian_log_prob(actions, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    cols = (obs, priv, actions, val, adv, ret, lp_o, mu_o, sg_o)
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    pd = P.Params(_dbl(p.actor), _dbl(p.critic), p.std.double())
    sel = [t[idx].double() for t in cols]
    if unclipped:       # (R - V)^2: the clipped form with the old values AT the returns' far side never clips -- restated directly instead
        sel[3] = sel[5].clone()      # old values = returns: v_clipped = R + clamp(V - R), l2 <= l1 always, so max(l1, l2) = l1 = (V - R)^2
    want = P.ppo_loss_and_grads(pd, *sel, quant=_q64)
    kw = {}
    if xb16:
        sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(torch.bfloat16).cuda().contiguous()
        kw = dict(obs_bf16=sh(obs, net.shadow_ld(0)), priv_bf16=sh(priv, net.shadow_ld(1)))
    net.ppo_grad(make_ppo_config(clipped_value_loss=not unclipped), make_batch(*[t.cuda().contiguous() for t in cols], idx.cuda(), **kw))
    torch.cuda.synchronize()
    errs = {k: _rel_l2(got.cpu(), r) for k, got, r in zip(net.views, _split(net, net.grads), want["grads"].tensors())}
    kb = "critic.6.bias"        # one number, a cancelling sum: against the size of its terms (tests/test_activations_gpu.py)
    got_b = _split(net, net.grads)[list(net.views).index(kb)].cpu().double()
    errs[kb] = float((got_b - want["grads"].tensors()[list(net.views).index(kb)].double()).norm() / want["d_val"].double().norm())
    worst = max(errs, key=errs.get)
    BR.check("fused gradient %s %s %s%s vs restated reference (worst tensor: %s)" % (name, shape, "shadow" if xb16 else "fp32 rows",
                                                                                    ", unclipped" if unclipped else "", worst), errs[worst], GRAD_TOL)
    np.testing.assert_allclose(float(net.opt_state[L.OPT_VALUE_SUM]), float(want["value_loss"]), rtol=1e-2)


# ---------------------------------------------------------------------------------------------- 5. auxiliary head
def test_auxiliary_head_under_tanh():
    """Tanh, aux_hidden = [512, 256, 128], aux_out = 32, flag on: forward(2) at the forward bars, and the denoiser.* gradients of a
    ppo_grad with aux_coef > 0 at the gradient bar against torch float64 autograd of the restated (bf16-rounding) forward."""
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch
    act = nn.Tanh()
    fwd, _ = LP.restated(act)
    S, B, coef, OFF = 900, 700, 0.5, 219 - 32
    g = torch.Generator().manual_seed(13)
    p = P.Params.random(705, 219, 12, [512, 256, 128], [768, 256, 128], g)
    den = P.Params.random(705, 219, 32, [512, 256, 128], [8], g).actor
    net = NetBuffers(make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], "bf16", S, aux_hidden=[512, 256, 128], aux_out=32,
                                     aux_target_offset=OFF, activation=act, fused_activation=True), "cuda")
    net.load_state_dict(dict(zip(list(net.views), list(p.tensors()) + [t for W, b in den for t in (W, b)])))
    assert net.shadow_ld(0) > 0
    obs, priv = torch.randn(S, 705, generator=g) * 2, torch.randn(S, 219, generator=g)
    with torch.no_grad():
        ref = fwd(obs.double(), _dbl(den), quant=_q64)
    y = net.forward(2, obs.cuda())
    torch.cuda.synchronize()
    d = y.cpu().double() - ref
    BR.check("fused denoiser head tanh forward, rel-L2", float(d.norm() / ref.norm()), FWD_TOL)
    BR.check("fused denoiser head tanh forward, worst output", float(d.abs().max() / ref.abs().max()), FWD_MAX_TOL)
    r = lambda *s: torch.randn(*s, generator=g)
    cols = (obs, priv, r(S, 12), r(S), r(S), r(S), r(S) - 12.0, r(S, 12) * 0.3, torch.ones(S, 12))
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    net.ppo_grad(make_ppo_config(aux_coef=coef), make_batch(*[t.cuda().contiguous() for t in cols], idx.cuda()))
    torch.cuda.synchronize()
    # float64 autograd through the bf16-rounding forward with a straight-through rounding (the kernels' dZ is the gradient of the
    # rounded values), derivative of tanh from the rounded y
    layers = [(W.double().requires_grad_(), b.double().requires_grad_()) for W, b in den]
    st = lambda t: t + (_q64(t) - t).detach()
    h = _q64(obs[idx].double())
    for i, (W, b) in enumerate(layers):
        z = torch.nn.functional.linear(h, st(W), b)
        if i < 3:
            yq = _q64(torch.tanh(z)).detach()
            h = yq + (z - z.detach()) * (1.0 - yq * yq)      # value yq, derivative 1 - yq^2
        else:
            h = z
    mse = ((h - priv[idx].double()[:, OFF:OFF + 32]) ** 2).mean()
    (coef * mse).backward()
    np.testing.assert_allclose(float(net.opt_state[L.OPT_AUX_SUM]), float(mse.detach()), rtol=1e-2)
    gv = net.grad_views()
    errs = {}
    for l, (W, b) in enumerate(layers):
        errs["denoiser.%d.weight" % (2 * l)] = _rel_l2(gv["denoiser.%d.weight" % (2 * l)].cpu(), W.grad)
        errs["denoiser.%d.bias" % (2 * l)] = _rel_l2(gv["denoiser.%d.bias" % (2 * l)].cpu(), b.grad)
    worst = max(errs, key=errs.get)
    BR.check("fused denoiser head tanh gradient vs float64 autograd (worst tensor: %s)" % worst, errs[worst], GRAD_TOL)


# ---------------------------------------------------------------------------------------------- 6. rollout, 7. evaluation, 8. runner
def _runner(num_envs, seed, activation, monkeypatch, steps=None):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    import copy
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    _, train_cfg = task_registry.get_cfgs(name=args.task)
    train_cfg = copy.deepcopy(train_cfg)
    train_cfg.seed = seed
    if steps:
        train_cfg.runner.num_steps_per_env = steps
    import sys
    from humanoid.algo import OnPolicyRunner
    R = sys.modules[OnPolicyRunner.__module__]
    AC = getattr(R, "_fa_AC", None) or R.ActorCritic
    monkeypatch.setattr(R, "_fa_AC", AC, raising=False)
    # what train_cfg["policy"]["activation"] / ["fused_activation"] do: the runner passes **policy_cfg into ActorCritic (the config
    # classes are flattened by class_to_dict, which would take a module apart, so the module is handed in at the constructor)
    monkeypatch.setattr(R, "ActorCritic", lambda *a, **k: AC(*a, **dict(k, activation=activation, fused_activation=True)))
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg, log_root=None)
    return runner


@pytest.mark.parametrize("num_envs", [256, 64])
@pytest.mark.parametrize("name", ["relu", "sigmoid"])
def test_fused_rollout_step_equals_act_then_step(name, num_envs, monkeypatch):
    """hgym_rollout_step on a flag-on net (one launch per vec-step, 6 steps, episode lengths staggered so that resets occur; 64 envs: a
    last partial pair of tiles) against PPO.act + env.step on the same net and seeds: storage, env state, the bf16 shadows (which
    include the columns the carried first layer wrote ahead) and the parameters after the update bit-identical -- the comparison
    tests/test_fused_gpu.py::test_fused_rollout_step_equals_act_then_step makes for ELU(1)."""
    from humanoid.algo import PPO
    monkeypatch.setattr(PPO, "precision", "bf16")
    monkeypatch.setenv("HGYM_GRAPH", "0")
    outs = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("HGYM_FUSE_ROLLOUT", fuse)
        torch.manual_seed(4321)
        np.random.seed(4321)
        r = _runner(num_envs, 31, ACTS[name], monkeypatch, steps=6)
        assert r.alg.net.shadow_ld(0) == 768 and r.env.rollout_fused_mode(r.alg.net) is not None
        r.env.episode_length_buf = 2400 - 2 - (torch.arange(num_envs, device="cuda") % 5)       # time-outs at steps 1 .. 5 of every rollout
        r.env._buf.counters[L.CNT_STEP] = 398                                                            # a push (every 400 steps) too
        r.learn(num_learning_iterations=2, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        st, b = r.alg.storage, r.env._buf
        assert int(st.dones.sum()) > 0
        outs[fuse] = dict(params=r.alg.net.params.clone(), obs=st._obs_all.clone(), priv=st._priv_all.clone(), rewards=st.rewards.clone(),
                          actions=st.actions.clone(), values=st.values.clone(), logp=st.actions_log_prob.clone(), mu=st.mu.clone(),
                          dones=st.dones.clone(), returns=st.returns.clone(), sample_step=r.alg._sample_step.clone(),
                          obs_bf16=st._obs_bf16.clone(), priv_bf16=st._priv_bf16.clone(),
                          state=b._state.clone(), root=b.root.clone(), dof_pos=b.dof_pos.clone(), dof_vel=b.dof_vel.clone(),
                          contact=b.contact.clone(), rigid=b.rigid.clone(), obs_ring=b.obs_ring.clone(), priv_ring=b.priv_ring.clone(),
                          ep_len=b.episode_length.clone(), counters=b.counters.clone(), rew=b.rew.clone(), reset=b.reset.clone(),
                          time_out=b.time_out.clone(), extras_time_outs=b.extras_time_outs.clone(), episode_acc=b.episode_acc.clone(),
                          env_obs=r.env.obs_buf.clone())
        assert torch.isfinite(outs[fuse]["params"]).all()
        extras = b.extras_episode.clone()
        del r
        outs[fuse]["extras_episode"] = extras
    for k in outs["1"]:
        if k == "extras_episode":        # means over resetting envs: fp32 atomics, order-dependent in the last bit (tests/test_fused_gpu.py)
            np.testing.assert_allclose(outs["1"][k].cpu().numpy(), outs["0"][k].cpu().numpy(), rtol=1e-5, atol=1e-9)
        else:
            assert torch.equal(outs["1"][k], outs["0"][k]), k


def test_fused_evaluation_equals_the_two_launch_path(monkeypatch):
    """Tanh, flag on, 256 envs, 4 steps: eval_rollout_supported, and evaluate(fused=True) returns the dict of fused=False bit for bit."""
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    monkeypatch.setattr(PPO, "precision", "bf16")
    r = _runner(256, 12, ACTS["tanh"], monkeypatch)
    res = {}
    for fused in (True, False):
        torch.manual_seed(22)
        np.random.seed(22)
        args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", "256", "--seed", "22"])
        env = task_registry.make_env(name=args.task, args=args)[0]
        env.reset()
        env.episode_length_buf = 2400 - 1 - (torch.arange(256, device="cuda") % 4)      # episodes end inside the window
        assert env.eval_rollout_supported(r.alg.net)
        res[fused] = r.evaluate(env, 4, reset=False, fused=fused)
    a, b = res[True], res[False]
    assert a["episodes"] > 0
    for k in a:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


@pytest.mark.parametrize("name", ["leaky0.01", "tanh"])
def test_runner_trains_and_captured_update_equals_eager(name, monkeypatch, tmp_path):
    """256 envs, bf16, flag on, three iterations: the rollout graph and the update graph both in use; the captured update and the eager
    one (HGYM_GRAPH_UPDATE=0) bit-identical in parameters, Adam moments and optimiser scalars, everything finite; the device inference
    policy against the JIT-exported CPU policy within BF16_BAR."""
    from humanoid.algo import PPO
    from humanoid.utils.helpers import export_policy_as_jit
    monkeypatch.setattr(PPO, "precision", "bf16")
    act = ACTS[name]
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", mode)
        torch.manual_seed(4321)
        np.random.seed(4321)
        r = _runner(256, 78, act, monkeypatch)
        alg = r.alg
        assert alg.actor_critic.fused_activation is True and alg.net.cfg.fused_activation == 1
        assert alg.net.shadow_ld(0) == 768 and alg.net.shadow_ld(1) == 256
        assert r.env.rollout_fused_mode(alg.net) is not None and r.env.eval_rollout_supported(alg.net) and alg.update_capturable()
        r.env.episode_length_buf = torch.arange(256, device="cuda") * 7
        r.learn(num_learning_iterations=3, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        assert (r._update_graph is not None) == (mode == "1") and r._graph is not None
        assert int(alg.net.opt_state[L.OPT_STEP]) == 3 * alg.num_learning_epochs * alg.num_mini_batches
        opt = alg.net.opt_state.clone()
        assert torch.isfinite(opt[:L.OPT_GRAD_SQNORM]).all() and torch.isfinite(alg.net.params).all()
        if float(opt[L.OPT_GRAD_SQNORM]) >= 128.0:      # fp64 atomics beyond their exact range (tests/test_fused_gpu.py)
            opt[L.OPT_GRAD_SQNORM] = 0.0
        outs[mode] = (alg.net.params.clone(), alg.net.adam_m.clone(), alg.net.adam_v.clone(), opt)
        if mode == "0":
            policy = r.get_inference_policy()
            obs = (torch.randn(512, 705) * 2).clamp(-18, 18)
            with torch.no_grad():
                dev = policy(obs.cuda()).cpu().double()
            export_policy_as_jit(alg.actor_critic, str(tmp_path))
            jit = torch.jit.load(str(tmp_path / "policy_1.pt"))
            with torch.no_grad():
                cpu = jit(obs).double()
            BR.check("fused runner %s: device inference policy vs JIT-exported CPU policy (fp32), rel-L2" % name, _rel_l2(dev, cpu), BR.BF16_BAR)
        del r
    for nm, a, b in zip(("params", "adam_m", "adam_v", "opt_state"), outs["1"], outs["0"]):
        assert torch.equal(a, b), nm


def test_critic_values_over_more_rows_than_max_batch():
    """hgym_critic_values on a flag-on Sigmoid net: 300 rows in pieces of max_batch = 128, values at the forward bars, the bf16 shadow rows
    it leaves equal to the rounded input."""
    act = ACTS["sigmoid"]
    p, net, g = _setup(act, "xbotl", 128, 51)
    fwd, _ = LP.restated(act)
    priv = (torch.randn(300, 219, generator=g) * 2).clamp(-18, 18)
    with torch.no_grad():
        ref = fwd(priv.double(), _dbl(p.critic), quant=_q64).squeeze(-1)
    x, v = priv.cuda(), torch.empty(300, device="cuda")
    sh = torch.zeros(300, net.shadow_ld(1), dtype=torch.bfloat16, device="cuda")
    net.critic_values(x, v, priv_bf16=sh)
    torch.cuda.synchronize()
    d = v.cpu().double() - ref
    BR.check("fused critic_values sigmoid, rel-L2", float(d.norm() / ref.norm()), FWD_TOL)
    BR.check("fused critic_values sigmoid, worst output", float(d.abs().max() / ref.abs().max()), SIGMOID_FWD_MAX_TOL)
    assert torch.equal(sh[:, :219], x.to(torch.bfloat16)) and (sh[:, 219:] == 0).all()


# ---------------------------------------------------------------------------------------------- 9. ELU(1) untouched
def test_elu1_flag_changes_nothing():
    """nn.ELU() with the flag on and off: one forward of each net and one ppo_grad, torch.equal on outputs and gradients."""
    from hgym import make_ppo_config, make_batch
    S, B = 700, 600
    res = []
    for flag in (False, True):
        p, net, g = _setup(nn.ELU(), "xbotl", S, 41, fused_activation=flag)
        assert net.shadow_ld(0) == 768
        r = lambda *s: torch.randn(*s, generator=g)
        cols = (r(S, 705), r(S, 219), r(S, 12), r(S), r(S), r(S), r(S) - 12.0, r(S, 12) * 0.3, torch.ones(S, 12))
        idx = torch.randperm(S, generator=g)[:B].contiguous()
        y0, y1 = net.forward(0, cols[0].cuda()), net.forward(1, cols[1].cuda())
        net.ppo_grad(make_ppo_config(), make_batch(*[t.cuda().contiguous() for t in cols], idx.cuda()))
        torch.cuda.synchronize()
        res.append((y0.clone(), y1.clone(), net.grads_ext.clone(), net.opt_state.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
