"""-m gpu: the first-layer loops of the fused bf16 kernels run ceil(K / 32) k-steps while every buffer stays padded to 128 columns
(csrc/hgym_fused.hpp: l0_ksteps, mma_chunk_last).  A last chunk of 1, 2, 3 and 4 k-steps, widths exactly on a k-step and on a chunk
edge and the two production widths, through the forward (mlp_fwd_kernel, fp32 input rows), the update tiles on fp32 rows and on the
bf16 shadow (mlp_fb_kernel, both staging paths) and the rollout launch in its 64-row layout (the actor tiles run the short loop from
the carried k-steps on; the 64-row critic tiles keep all padded k-steps, csrc/hgym_fused.hpp: L0_FULL).

The last valid input column of every case carries a weight of +-2 (the other weights are below 1 / sqrt(K) <= 0.11) and an input of 1.5:
a k-step dropped too early removes +-3 from every first-layer pre-activation."""
import copy

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as P
from oracle import xbot_constants as XK
from hgym import _lib as L

pytestmark = pytest.mark.gpu
NAMES = ["std"] + ["actor.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")] + \
        ["critic.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")]
WIDTHS = [97, 128, 129, 160, 161, 219, 224, 225, 705]       # nlast = 4, 4, 1, 1, 2, 3, 3, 4, 3
BATCHES = [1, 64, 65, 96]
# the bounds tests/test_fused_gpu.py::test_fused_and_generic_bf16_paths_agree holds the two bf16 paths to
FWD_TOL = 1e-2
GRAD_COS = 0.999


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _case(K, M):
    g = torch.Generator().manual_seed(1000 * K + M)
    p = P.Params.random(K, K, 12, XK.ACTOR_HIDDEN, XK.CRITIC_HIDDEN, g)
    for layers in (p.actor, p.critic):
        W0 = layers[0][0]
        W0[:, K - 1] = 2.0 * (1.0 - 2.0 * (torch.arange(W0.shape[0]) % 2))
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    obs, priv = torch.randn(M, K, generator=g).clamp(-18, 18), torch.randn(M, K, generator=g).clamp(-18, 18)
    obs[:, K - 1] = 1.5
    priv[:, K - 1] = 1.5
    z = torch.randn(M, 12, generator=g)
    act, mu_o = torch.randn(M, 12, generator=g), torch.randn(M, 12, generator=g) * 0.3
    sg_o = torch.rand(M, 12, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(M, generator=g), torch.randn(M, generator=g), torch.randn(M, generator=g)
    with torch.no_grad():
        mu_now = P.mlp_forward(obs, p.actor)
    # old log-probabilities next to the current ones (ratio ~ 1) and a clip range that never binds: the surrogate is smooth in mu, so
    # the two paths' bf16 rounding cannot put a sample on different sides of a clip edge (tests/test_fused_gpu.py:103-108)
    lp_o = P.gaussian_log_prob(act, mu_now, mu_now * 0 + p.std) + torch.randn(M, generator=g) * 0.1
    idx = torch.arange(M)
    c = lambda t: t.cuda().contiguous()
    return p, c(obs), c(priv), c(z), [c(t) for t in (act, val, adv, ret, lp_o, mu_o, sg_o, idx)]


def _run_path(K, M, p, obs, priv, z, cols, shadow):
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch
    net = NetBuffers(make_net_config(K, K, 12, XK.ACTOR_HIDDEN, XK.CRITIC_HIDDEN, "bf16", max(M, 64)), "cuda", learning_rate=1e-3)
    net.load_state_dict(dict(zip(NAMES, p.tensors())))
    ppo = make_ppo_config(clip_param=100.0)
    sh = None
    if shadow:
        ld = (net.shadow_ld(0), net.shadow_ld(1))
        assert ld == ((K + 127) // 128 * 128,) * 2
        sh = tuple(torch.full((M, l), 7.0, dtype=torch.bfloat16, device="cuda") for l in ld)
    out = net.act(obs, priv, z=z, shadow=sh)
    net.ppo_grad(ppo, make_batch(obs, priv, *cols))
    torch.cuda.synchronize()
    res = dict(mu=out["mu"].clone(), values=out["values"].clone(), grads=net.grads[:net.P].clone())
    if shadow:
        for s, x in zip(sh, (obs, priv)):           # the policy launch's shadow: the row's bf16, every pad column zero
            assert torch.equal(s[:, :K], x.to(torch.bfloat16)) and float(s[:, K:].float().abs().max() if s.shape[1] > K else 0.0) == 0.0
        net.grads_ext.zero_()
        net.ppo_grad(ppo, make_batch(obs, priv, *cols, obs_bf16=sh[0], priv_bf16=sh[1]))
        torch.cuda.synchronize()
        res["grads_shadow"] = net.grads[:net.P].clone()
    return res


@pytest.mark.parametrize("M", BATCHES)
@pytest.mark.parametrize("K", WIDTHS)
def test_fused_first_layer_vs_layer_by_layer_path(monkeypatch, K, M):
    """net.act and net.ppo_grad of the fused bf16 path against the layer-by-layer bf16 path (HGYM_NO_FUSED=1) on the same parameters and
    rows, actor and critic both with a first layer of width K: forward within 1e-2 of the output scale, gradient cosine > 0.999 (the
    suite's bounds for this pair of paths).  The update from the bf16 shadow the policy launch wrote must equal the update from the fp32
    rows bit for bit, as tests/test_fused_gpu.py::test_update_from_the_bf16_shadow_equals_update_from_fp32_rows has it at 705 / 219."""
    p, obs, priv, z, cols = _case(K, M)
    monkeypatch.delenv("HGYM_NO_FUSED", raising=False)
    fused = _run_path(K, M, p, obs, priv, z, cols, shadow=True)
    monkeypatch.setenv("HGYM_NO_FUSED", "1")
    layer = _run_path(K, M, p, obs, priv, z, cols, shadow=False)
    monkeypatch.delenv("HGYM_NO_FUSED")
    e_mu, e_v = _rel(fused["mu"].cpu(), layer["mu"].cpu()), _rel(fused["values"].cpu(), layer["values"].cpu())
    a, b = fused["grads"].double(), layer["grads"].double()
    cos = float(a @ b) / float(a.norm() * b.norm())
    print("K=%d M=%d: mu %.3e  values %.3e  gradient cosine %.6f" % (K, M, e_mu, e_v, cos))
    assert torch.isfinite(fused["grads"]).all() and float(a.norm()) > 0.0
    assert e_mu <= FWD_TOL and e_v <= FWD_TOL, (e_mu, e_v)
    assert cos > GRAD_COS, cos
    assert torch.equal(fused["grads_shadow"], fused["grads"])


# ---------------------------------------------------------------------------------------------- the rollout launch
def _runner(num_envs, seed, steps):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    _, train_cfg = task_registry.get_cfgs(name=args.task)
    train_cfg = copy.deepcopy(train_cfg)
    train_cfg.seed = seed
    train_cfg.runner.num_steps_per_env = steps
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg, log_root=None)
    return runner


@pytest.mark.parametrize("kb0", [None, "12"])
def test_rollout_64_row_layout_equals_act_then_step(monkeypatch, kb0):
    """hgym_rollout_step in the 64-row layout (128 envs, the fewest it takes: four actor tiles, two 64-row critic tiles, two side-job workgroups), 3 steps a
    rollout, the actor's first layer carried over kb0 = 20 (default) or 12 k-steps -- the actor tile then runs k-steps [kb0, 23) of 24 --
    against PPO.act + env.step (tests/test_fused_gpu.py::test_fused_rollout_step_equals_act_then_step): storage, values, bf16 shadows,
    env state and the parameters after four iterations bit-identical, every pad column of the shadows zero."""
    from humanoid.algo import PPO
    monkeypatch.setattr(PPO, "precision", "bf16")
    monkeypatch.setenv("HGYM_GRAPH", "0")
    monkeypatch.setenv("HGYM_RO_CRITIC64", "1")
    if kb0 is None:
        monkeypatch.delenv("HGYM_L0_KB0", raising=False)
    else:
        monkeypatch.setenv("HGYM_L0_KB0", kb0)
    N, outs = 128, {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("HGYM_FUSE_ROLLOUT", fuse)
        torch.manual_seed(4321)
        np.random.seed(4321)
        r = _runner(N, 31, 3)
        assert (r.alg.net.shadow_ld(0), r.alg.net.shadow_ld(1)) == (768, 256)
        assert (r.env.rollout_fused_mode(r.alg.net) is not None) or fuse == "0"
        # every fourth env times out within the first rollouts (its carried sums are dropped); the others keep their history, so that
        # after four rollouts 12 of the 15 frames -- columns inside the first 12 k-steps among them -- are non-zero
        i = torch.arange(N, device="cuda")
        r.env.episode_length_buf = torch.where(i % 4 == 0, 2400 - 2 - (i // 4) % 5, 0 * i)
        r.learn(num_learning_iterations=4, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        st, b = r.alg.storage, r.env._buf
        assert int(st.dones.sum()) > 0
        if fuse == "1":
            assert b._l0_partial is not None and bool((b._l0_partial != 0).any())          # the hand-over really ran
        outs[fuse] = dict(params=r.alg.net.params.clone(), obs=st._obs_all.clone(), priv=st._priv_all.clone(), rewards=st.rewards.clone(),
                          actions=st.actions.clone(), values=st.values.clone(), logp=st.actions_log_prob.clone(), mu=st.mu.clone(),
                          dones=st.dones.clone(), returns=st.returns.clone(), obs_bf16=st._obs_bf16.clone(), priv_bf16=st._priv_bf16.clone(),
                          state=b._state.clone(), obs_ring=b.obs_ring.clone(), priv_ring=b.priv_ring.clone(), ep_len=b.episode_length.clone(),
                          counters=b.counters.clone(), env_obs=r.env.obs_buf.clone())
        del r
    for k in outs["1"]:
        assert torch.equal(outs["1"][k], outs["0"][k]), k
    assert torch.isfinite(outs["1"]["params"]).all()
    for k, width in (("obs_bf16", 705), ("priv_bf16", 219)):
        sh = outs["1"][k]
        sh = sh.reshape(-1, sh.shape[-1])
        assert sh.shape[-1] in (768, 256) and float(sh[:, width:].float().abs().max()) == 0.0, k
        assert float(sh[:, :width].float().abs().max()) > 0.0
