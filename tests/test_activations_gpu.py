"""-m gpu: every supported hidden-layer activation (HgymNetConfig.activation) through the HIP path, against float64 references restated
here for activations other than ELU (oracle/ppo_oracle.py implements ELU(1) only).

The fused bf16 kernels implement ELU(1) only; a bf16 net with any other activation runs the layer-by-layer GEMM path (hgym_gemm.hpp:
act_fwd_tile / act_bwd_tile), at every width, and the rollout falls back from hgym_rollout_step to PPO.act + the env step.  The restated
references follow the oracle's conventions: with quant = bf16 rounding, operands and every hidden activation y are rounded where the
kernels round, dZ is rounded where it is stored, and the derivative is taken from the ROUNDED y, as the kernels take it."""

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
# bars: the ones tests/test_fused_shapes_gpu.py (bf16) and tests/test_net_gpu.py (fp32 parity) hold for ELU
FWD_TOL, FWD_MAX_TOL = 2e-3, 5e-3       # bf16 forward: rel-L2 over all rows, worst single output / output scale
GRAD_TOL = 5e-3                         # bf16 gradient, per tensor, rel-L2
F32_FWD_TOL = 1e-5                      # fp32 forward vs float64, rel-L2 and worst output / scale
F32_GRAD_TOL = 5e-5                     # fp32 gradient, per tensor (tests/test_net_gpu.py's parity bar)
# Sigmoid, worst single output: every hidden y of a sigmoid net lies near 0.5, so where the kernel's fp32 pre-activation and the float64
# one fall on two sides of a bf16 rounding boundary, y moves by 2^-9 x ~0.5 -- several times the typical flip of an ELU / tanh net, whose
# y cluster near 0.  Measured: 2.2e-3 and 1.05e-2 on two critics of XBot-L's widths [768, 256, 128] (different weights), rel-L2 <= 2e-3
# on both.  The worst-output bar for sigmoid is 2e-2 (a wrong row is off by the output scale itself, ~1); rel-L2 keeps FWD_TOL.
SIGMOID_FWD_MAX_TOL = 2e-2
SHAPES = {
    "xbotl": ([512, 256, 128], [768, 256, 128]),
    "256x3": ([256, 256, 256], [256, 256, 256]),
    "big_actor": ([768, 256, 128], [768, 256, 128]),     # refused by the fused tiles even at ELU(1)
}


def _restated(m):
    """mlp_forward / mlp_backward of oracle/ppo_oracle.py with the activation m in place of ELU(1) (tests/layer_path_common.py)."""
    return LP.restated(m)


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


def _setup(act, shape, precision, max_batch, seed, **kw):
    from hgym import NetBuffers, make_net_config
    ah, ch = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    p = P.Params.random(705, 219, 12, ah, ch, g)
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    net = NetBuffers(make_net_config(705, 219, 12, ah, ch, precision, max_batch, activation=act, **kw), "cuda", learning_rate=1e-3)
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    return p, net, g


CASES = [(a, s, "bf16") for a in ACTS for s in SHAPES] + [(a, "xbotl", "f32") for a in ACTS]
IDS = ["%s-%s-%s" % c for c in CASES]


@pytest.mark.parametrize("name,shape,precision", CASES, ids=IDS)
def test_forward_vs_restated_reference(name, shape, precision, monkeypatch):
    """hgym_mlp_forward of the actor and the critic, M = 1, 100 and 5000 rows."""
    act = ACTS[name]
    M = 5000
    p, net, g = _setup(act, shape, precision, M, 11)
    assert net.shadow_ld(0) == 0                 # not the fused path: it implements ELU(1) only
    fwd, _ = _restated(act)
    q = _q64 if precision == "bf16" else None
    obs = (torch.randn(M, 705, generator=g) * 2).clamp(-18, 18)
    priv = (torch.randn(M, 219, generator=g) * 2).clamp(-18, 18)
    with torch.no_grad():
        ref = {0: fwd(obs.double(), _dbl(p.actor), quant=q), 1: fwd(priv.double(), _dbl(p.critic), quant=q)}
    xs = {0: obs.cuda(), 1: priv.cuda()}
    tol, tol_max = (FWD_TOL, SIGMOID_FWD_MAX_TOL if name == "sigmoid" else FWD_MAX_TOL) if precision == "bf16" else (F32_FWD_TOL, F32_FWD_TOL)
    for m in (1, 100, M):
        for which in (0, 1):
            y = net.forward(which, xs[which][:m].contiguous())
            torch.cuda.synchronize()
            d, r = y.cpu().double() - ref[which][:m], ref[which][:m]
            what = "forward %s %s %s %s, M = %d vs restated reference" % (name, shape, precision, ("actor", "critic")[which], m)
            BR.check(what + ", rel-L2", float(d.norm() / r.norm()), tol)
            BR.check(what + ", worst output", float(d.abs().max() / ref[which].abs().max()), tol_max)


@pytest.mark.parametrize("name,shape,precision", CASES, ids=IDS)
def test_gradient_vs_restated_reference(name, shape, precision, monkeypatch):
    """hgym_ppo_grad on one minibatch (S = 5000 stored rows, B = 4096) against the oracle's PPO loss and backward with the restated
    MLP, per parameter tensor."""
    from hgym import make_ppo_config, make_batch
    act = ACTS[name]
    S, B = 5000, 4096
    p, net, g = _setup(act, shape, precision, B, 12)
    fwd, bwd = _restated(act)
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
    want = P.ppo_loss_and_grads(pd, *(t[idx].double() for t in cols), quant=_q64 if precision == "bf16" else None)
    net.ppo_grad(make_ppo_config(), make_batch(*[t.cuda().contiguous() for t in cols], idx.cuda()))
    torch.cuda.synchronize()
    errs = {k: _rel_l2(got.cpu(), r) for k, got, r in zip(net.views, _split(net, net.grads), want["grads"].tensors())}
    # critic.6.bias is ONE number, the sum of the B per-sample value-loss gradients d_val, which cancel to a small fraction of their size
    # (mean of (V - R) over the batch); relative to itself its error is ill-conditioned (measured 4.3e-2 under tanh, with the tensor at a
    # few 1e-3).  It is measured against the size of its terms instead, ||d_val||_2 -- what a sum of B random-sign terms amounts to.
    kb = "critic.6.bias"
    got_b = _split(net, net.grads)[list(net.views).index(kb)].cpu().double()
    errs[kb] = float((got_b - want["grads"].tensors()[list(net.views).index(kb)].double()).norm() / want["d_val"].double().norm())
    worst = max(errs, key=errs.get)
    BR.check("gradient %s %s %s vs restated reference (worst tensor: %s)" % (name, shape, precision, worst), errs[worst],
             GRAD_TOL if precision == "bf16" else F32_GRAD_TOL)
    opt = net.opt_state.cpu()
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM]), float(want["value_loss"]), rtol=1e-2)


def test_denoiser_head_under_tanh():
    """The auxiliary (denoising) head takes the configuration's activation: hgym_mlp_forward(which = 2) under nn.Tanh() against the
    restated reference, bf16 and fp32."""
    act = nn.Tanh()
    fwd, _ = _restated(act)
    for precision in ("bf16", "f32"):
        from hgym import NetBuffers, make_net_config
        g = torch.Generator().manual_seed(13)
        p = P.Params.random(705, 219, 12, [512, 256, 128], [768, 256, 128], g)
        den = P.Params.random(705, 219, 32, [512, 256, 128], [8], g).actor      # an MLP 705 -> 512 -> 256 -> 128 -> 32
        net = NetBuffers(make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], precision, 2000, aux_hidden=[512, 256, 128],
                                         aux_out=32, aux_target_offset=219 - 32, activation=act), "cuda")
        names = [k for k in net.views if k.startswith("denoiser.")]
        assert len(names) == 8
        net.load_state_dict(dict(zip(list(net.views), list(p.tensors()) + [t for W, b in den for t in (W, b)])))
        layers = den
        obs = torch.randn(2000, 705, generator=g) * 2
        with torch.no_grad():
            ref = fwd(obs.double(), _dbl(layers), quant=_q64 if precision == "bf16" else None)
        y = net.forward(2, obs.cuda())
        torch.cuda.synchronize()
        d = y.cpu().double() - ref
        tol = FWD_TOL if precision == "bf16" else F32_FWD_TOL
        BR.check("denoiser head tanh %s forward, rel-L2" % precision, float(d.norm() / ref.norm()), tol)


def _runner(num_envs, seed, activation, monkeypatch):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    tc = task_registry.train_cfgs[args.task]
    tc.seed = seed
    # what train_cfg["policy"]["activation"] does: the runner passes **policy_cfg into ActorCritic (the config classes are flattened by
    # class_to_dict, which would take a module apart, so the module is handed in at the constructor here)
    import sys
    from humanoid.algo import OnPolicyRunner
    R = sys.modules[OnPolicyRunner.__module__]
    AC = R.ActorCritic
    monkeypatch.setattr(R, "ActorCritic", lambda *a, **k: AC(*a, **dict(k, activation=activation)))
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    return runner


@pytest.mark.parametrize("name", ["leaky0.01", "tanh"])
def test_runner_trains_and_captured_update_equals_eager(name, monkeypatch, tmp_path):
    """make_alg_runner / learn with train_cfg["policy"]["activation"] set, 256 envs, bf16: three iterations with the update replayed from
    its HIP graph and three issued eagerly (HGYM_GRAPH_UPDATE=0), same seeds: finite, and parameters, Adam moments and optimiser scalars
    bit-identical.  The runner takes PPO.act + the env step (the fused rollout step needs the fused ELU(1) net).  Then the device's
    inference policy against the JIT-exported CPU policy, within the bf16 forward bar."""
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
        assert alg.actor_critic.activation is act and alg.net.cfg.activation == {"leaky0.01": 2, "tanh": 3}[name]
        assert alg.net.shadow_ld(0) == 0 and r.env.rollout_fused_mode(alg.net) is None
        r.env.episode_length_buf = torch.arange(256, device="cuda") * 7
        r.learn(num_learning_iterations=3, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        assert (r._update_graph is not None) == (mode == "1")
        assert int(alg.net.opt_state[L.OPT_STEP]) == 3 * alg.num_learning_epochs * alg.num_mini_batches
        opt = alg.net.opt_state.clone()
        assert torch.isfinite(opt[:L.OPT_GRAD_SQNORM]).all() and torch.isfinite(alg.net.params).all()
        if float(opt[L.OPT_GRAD_SQNORM]) >= 128.0:      # fp64 atomics beyond their exact range (tests/test_fused_gpu.py)
            opt[L.OPT_GRAD_SQNORM] = 0.0
        outs[mode] = (alg.net.params.clone(), alg.net.adam_m.clone(), alg.net.adam_v.clone(), opt)
        if mode == "0":
            policy = r.get_inference_policy()           # act_inference: the HIP forward
            obs = (torch.randn(512, 705) * 2).clamp(-18, 18)
            with torch.no_grad():
                dev = policy(obs.cuda()).cpu().double()
            export_policy_as_jit(alg.actor_critic, str(tmp_path))
            jit = torch.jit.load(str(tmp_path / "policy_1.pt"))
            assert [c.original_name for c in jit.children()][1] == type(act).__name__
            with torch.no_grad():
                cpu = jit(obs).double()
            # bf16 operands against the fp32 module: the project's bf16-vs-fp32 bar (bf16_report.BF16_BAR), not FWD_TOL, which
            # holds bf16 against the bf16-operand reference (measured 3.6e-3 / 3.4e-3 for leaky0.01 / tanh after three iterations)
            BR.check("runner %s: device inference policy vs JIT-exported CPU policy (fp32), rel-L2" % name, _rel_l2(dev, cpu), BR.BF16_BAR)
        del r
    for nm, a, b in zip(("params", "adam_m", "adam_v", "opt_state"), outs["1"], outs["0"]):
        assert torch.equal(a, b), nm
