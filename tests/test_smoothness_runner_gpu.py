"""-m gpu: the smoothness regulariser through the drop-in stack (PPO.smoothness, OnPolicyRunner's smoothness_cfg),
at 64 envs, rollouts of 8 steps, 2 minibatches x 2 epochs.

  * the captured update replays what the eager update does, bit for bit over 3 iterations, on every loop plan; update_graph_key() changes
    with a coefficient; Loss/smooth_* are finite and positive;
  * one combined case: RND, empirical_normalization, log std, the auxiliary head and per-minibatch advantages all on;
  * an exact resume from the middle continues bit for bit with both terms on;
  * slot T holds the bootstrap observation at update time on the stepwise path (given last_obs; refused by name without it) as on the
    fused one;
  * PPO with smoothness = None launches what the parent launches and has nothing of the feature; twenty Adam steps on either term alone
    lower that term's roughness; init_storage's refusals."""
import copy
import os

import numpy as np
import pytest
import torch

import smoothness_common as S
import update_options_common as U
import test_update_options_gpu as G
from hgym import _lib as L

pytestmark = pytest.mark.gpu
TASK, N, T = "humanoid_ppo", 64, 8
BOTH = dict(temporal_coef=2.0, spatial_coef=4.0)
# loop plans of the runner: the knobs OnPolicyRunner reads once per learn()
PLANS = {"default": {}, "unfused": {"HGYM_FUSE_ROLLOUT": "0"}, "no-rollout-graph": {"HGYM_GRAPH": "0"}, "sync": {"HGYM_ASYNC": "0"},
         "deferred-critic": {"HGYM_ROLLOUT_CRITIC": "deferred"}, "host-log": {"HGYM_LOG_SINK": "0"}}


def _runner(tmp=None, smooth=None, seed=31, exact=False, save_interval=50, combined=False):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    task = "humanoid_dwl_ppo" if combined else TASK      # (the task with the auxiliary denoising head)
    args = get_args(["--task=" + task, "--headless", "--num_envs", str(N), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=task))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4                 # 400-step episodes: resets (and time-outs) inside the rollouts
    train_cfg.runner.num_steps_per_env = T
    train_cfg.runner.save_interval = save_interval
    train_cfg.algorithm.num_learning_epochs, train_cfg.algorithm.num_mini_batches = 2, 2
    if exact:
        train_cfg.runner.exact_resume = True
    if smooth is not None:
        train_cfg.algorithm.smoothness_cfg = smooth
    if combined:
        train_cfg.algorithm.rnd_cfg = dict(weight=0.5, predictor_hidden_dims=[256, 128, 128], target_hidden_dims=[256, 128, 128])
        train_cfg.algorithm.advantage_normalization = "minibatch"
        train_cfg.policy.empirical_normalization = True
        train_cfg.policy.noise_std_type = "log"
    env, _ = task_registry.make_env(name=task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name=task, args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    assert (runner.alg._smooth is not None) == (smooth is not None) and PPO.smoothness is None
    return runner


def _state(runner):
    torch.cuda.synchronize()
    net, st, sm = runner.alg.net, runner.alg.storage, runner.alg._smooth
    out = [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(), st._obs_all[0].clone()]
    if sm is not None:
        out += [sm.sums.clone(), sm.next_weight.clone()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("plan", list(PLANS))
def test_captured_update_equals_eager_update(monkeypatch, tmp_path, plan):
    for k in ("HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_GRAPH", "HGYM_ASYNC", "HGYM_ROLLOUT_CRITIC", "HGYM_LOG_SINK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    a = _runner(tmp_path / "a", smooth=BOTH)
    assert a.alg._smooth.cfg["noise_std"] is not None and len(a.alg._smooth.cfg["noise_std"]) == a.env.num_obs      # the env's own sensor noise
    assert max(a.alg._smooth.cfg["noise_std"]) > 0.0
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    a.wait_for_saves()
    sa = _state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(tmp_path / "b", smooth=BOTH)
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    b.wait_for_saves()
    assert b._update_graph is None
    assert _same(sa, _state(b)), "plan %s: the captured update and the eager one differ" % plan
    print("plan %s: update graph %s, rollout graph %s" % (plan, a._update_graph is not None, a._graph is not None))
    if plan == "default":
        assert a._update_graph is not None and a.alg.update_capturable()
    log = b.alg._smooth.read_log(b.alg._log.split(b.alg.log_block().cpu()))
    print("Loss/smooth_temporal %.4e Loss/smooth_spatial %.4e valid_fraction %.3f" % (log["temporal"], log["spatial"], log["valid_fraction"]))
    assert np.isfinite(log["temporal"]) and log["temporal"] > 0 and np.isfinite(log["spatial"]) and log["spatial"] > 0
    assert 0.5 < log["valid_fraction"] <= 1.0
    key = a.alg.update_graph_key()
    a.alg._smooth.cfg["temporal_coef"] = 3.0
    assert a.alg.update_graph_key() != key      # another coefficient re-captures
    off = _runner().alg.update_graph_key()
    assert dict(off)["smoothness"] is None and dict(key)["smoothness"] is not None and [n for n, _ in off] == [n for n, _ in key]


def test_loss_keys_are_logged(monkeypatch, tmp_path):
    seen = {}
    r = _runner(tmp_path / "log", smooth=BOTH)
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)      # opens the writer
    r.wait_for_saves()
    if r.writer is not None:
        monkeypatch.setattr(r.writer, "add_scalar", lambda k, v, it: seen.setdefault(k, []).append(float(v)))
    r.learn(num_learning_iterations=3, init_at_random_ep_len=False)
    r.wait_for_saves()
    torch.cuda.synchronize()
    assert r.alg.last_smoothness is not None and set(r.alg.last_smoothness) == {"temporal", "spatial", "valid_fraction"}
    if r.writer is not None:
        for k in ("Loss/smooth_temporal", "Loss/smooth_spatial"):
            assert k in seen and all(np.isfinite(v) and v > 0 for v in seen[k]), (k, seen.get(k))


def test_everything_else_on(monkeypatch):
    monkeypatch.delenv("HGYM_GRAPH_UPDATE", raising=False)
    a = _runner(smooth=BOTH, combined=True)
    alg = a.alg
    assert alg._rnd is not None and alg._obs_norm is not None and alg._adv_mode == "minibatch" and alg._ppo_cfg.aux_coef > 0.0
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    sa = _state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(smooth=BOTH, combined=True)
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert _same(sa, _state(b))
    assert all(torch.isfinite(t.double()).all() for t in sa)
    block = b.alg.log_block().cpu()
    parts = b.alg._log.split(block)
    log = b.alg._smooth.read_log(parts)
    assert log["temporal"] > 0 and log["spatial"] > 0 and b.alg._rnd.read_log(parts)["Loss/rnd"] > 0      # both tails are read where they lie
    assert block.numel() == L.OPT_STATE + b.alg._rnd.LOG_DOUBLES + 4


def test_exact_resume_from_the_middle(tmp_path, monkeypatch):
    monkeypatch.delenv("HGYM_GRAPH_UPDATE", raising=False)
    u = _runner(tmp_path / "u", smooth=BOTH, exact=True, save_interval=1)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    r = _runner(tmp_path / "r", smooth=BOTH, exact=True, save_interval=50)
    r.load(os.path.join(u.log_dir, "model_1.pt"))
    assert r.current_learning_iteration == 2
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(_state(u), _state(r))


def test_slot_T_holds_the_bootstrap_observation():
    """Stepwise, on the env's own output tensors (add_transitions copies them in, slot T is never written): refused without last_obs,
    copied from it otherwise.  The runner's zero-copy rollouts write slot T themselves: after learn() slot 0 (the rotated slot T) is the
    env's current observation."""
    r = _runner(smooth=BOTH)
    env, alg, st = r.env, r.alg, r.alg.storage
    with torch.inference_mode():
        obs, priv = env.get_observations(), env.get_privileged_observations()
        for _ in range(T):
            obs, priv, rew, dones, infos = env.step(alg.act(obs.clone(), priv.clone()))
            alg.process_env_step(rew, dones, infos)
        assert not alg._slot_T_written
        with pytest.raises(RuntimeError, match="last_obs"):
            alg.compute_returns(priv)
        st._obs_all[T].fill_(float("nan"))
        alg.compute_returns(priv, last_obs=obs)
        torch.cuda.synchronize()
        assert torch.equal(st._obs_all[T], obs)
        alg.update(sync=True)
    assert alg.last_smoothness["temporal"] > 0 and np.isfinite(alg.last_smoothness["temporal"])
    assert torch.isfinite(alg.net.params).all()
    f = _runner(smooth=BOTH)
    f.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert f.alg._slot_T_written and torch.equal(f.alg.storage._obs_all[0], f.env.get_observations())


def test_off_means_absent_and_the_parents_launches(monkeypatch):
    r = _runner()
    alg, st = r.alg, r.alg.storage
    assert alg._smooth is None and alg.smoothness is None and alg._options == () and dict(alg.update_graph_key())["smoothness"] is None
    assert alg.log_block().numel() == alg.net.opt_state.numel() == L.OPT_STATE and list(alg._log.split(alg.log_block().cpu())) == ["opt"]
    calls = []
    monkeypatch.setattr(alg.net, "ppo_grad_smooth", lambda *a: calls.append("smooth"))
    grad = alg.net.ppo_grad
    monkeypatch.setattr(alg.net, "ppo_grad", lambda *a: (calls.append("plain"), grad(*a)))
    import hgym
    monkeypatch.setattr(hgym, "smooth_pairs", lambda *a: calls.append("pairs"))
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert calls == ["plain"] * (2 * 2 * 2)      # iterations x epochs x minibatches, nothing else
    # ... and an explicit None is the same run, bit for bit
    q = _runner(smooth=None)
    q.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    assert _same(_state(r), _state(q))


def test_init_storage_refusals():
    from humanoid.algo import PPO
    from humanoid.utils.symmetry import xbot_l_mirror
    r = _runner()
    ac = r.alg.actor_critic
    alg = PPO(ac, num_mini_batches=2, device=r.device)
    alg.smoothness = dict(temporal_coef=1.0)
    alg.symmetry = xbot_l_mirror(r.env.cfg)
    with pytest.raises(ValueError, match="symmetry"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.symmetry = None
    alg.smoothness = dict(spatial_coef=1.0)
    with pytest.raises(ValueError, match="needs noise_std"):      # a bare PPO has no env to take the noise from
        alg.init_storage(N, T, [705], [219], [12])
    alg.smoothness = dict(lamT=1.0)
    with pytest.raises(ValueError, match="unknown key lamT"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.smoothness = dict(temporal_coef=1.0)
    alg._world = 2
    with pytest.raises(ValueError, match="one rank"):
        alg.init_storage(N, T, [705], [219], [12])


# ---------------------------------------------------------------------------------------------- the terms lower the roughness
@pytest.mark.parametrize("term", ["temporal", "spatial"])
def test_twenty_steps_on_the_term_alone_lower_the_roughness(term):
    """Advantages 0, value and entropy coefficients 0, a fixed learning rate: twenty Adam steps on one term alone.  The roughness is
    measured in plain torch float64 from the net's parameters before and after: mean |mu(s_t) - mu(s_t+1)|^2 over undone rows, and mean
    |mu(s) - mu(s~)|^2 over the perturbed rows the device wrote in the first step."""
    import hgym
    import test_smoothness_gpu as TG
    opts = U.Options("bf16-fused", None, "scalar", False, False, False, True)
    base = S.case_of(opts)
    cols = list(base["cols"])
    cols[4] = torch.zeros_like(cols[4])
    case = dict(base, cols=cols, ppo=dict(base["ppo"], value_coef=0.0, entropy_coef=0.0))
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case, value_loss_coef=0.0, entropy_coef=0.0, adaptive=False)
    # Adam moves every parameter by about the learning rate per step whatever the gradient's size.  The spatial roughness starts near 1e-3
    # (the targets are one noise draw away), so the steps must be small beside it: 1e-5, for both terms (at the suite's 1e-3 twenty
    # steps move every weight by 2e-2 and throw the net far past the minimum, although each step's gradient is the reference's).
    net.opt_state[L.OPT_LR] = 1e-5
    lam = (S.LAM_T, 0.0) if term == "temporal" else (0.0, S.LAM_S)
    obs, idx = case["cols"][0], case["idx"]
    near = None

    def rough():
        params = {k: v.cpu() for k, v in net.state_dict().items()}
        if term == "temporal":
            return S.roughness(opts, params, case["stats"], obs[idx], obs[case["nxt"]], case["weight"])
        return S.roughness(opts, params, case["stats"], obs[idx], near, torch.ones(len(idx)))
    for step in range(20):
        _, _, _, pr = TG._grad(net, opts, case, ppo, True, lam=lam)
        if step == 0:
            near = pr[:case["B"], :obs.shape[1]].cpu().clone()
            before = rough()
        net.ppo_apply(ppo)
    torch.cuda.synchronize()
    after = rough()
    print("%s roughness: %.6e -> %.6e after 20 Adam steps on the term alone" % (term, before, after))
    assert np.isfinite(after) and after < before
