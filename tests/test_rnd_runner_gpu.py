"""-m gpu: Random Network Distillation through the drop-in stack (PPO.rnd, OnPolicyRunner's rnd_cfg), at 64 envs,
rollouts of 4 steps, 2 minibatches; the predictor and the target on the fused bf16 path ([256, 128, 128]) and on the layer path ([64, 32]).

  * weight 0: the policy's parameters, Adam state and the stored rewards are bit for bit those of a run without RND, while the predictor trains;
  * weight > 0: storage.rnd_error is the restatement (tests/rnd_common.py) of the two bound nets' forward() outputs, the stored rewards are
    extrinsic + intrinsic bitwise;
  * ten predictor steps on fixed stored rows lower the MSE;
  * the captured update replays what the eager update does, the three nets and the block included;
  * checkpoints carry rnd_state_dict, load() refuses both mismatches by name, and an exact resume (2 + 2 iterations) is the run of 4;
  * with the mirror loss on beside it, the log block holds both tails and each reader finds its own by name;
  * with PPO.rnd = None nothing of the feature exists."""
import copy
import os

import numpy as np
import pytest
import torch

import rnd_common as R
from hgym import _lib as L

pytestmark = pytest.mark.gpu
TASK, N, T = "humanoid_ppo", 64, 4
NETS = dict(fused=dict(predictor_hidden_dims=[256, 128, 128], target_hidden_dims=[256, 128, 128]),
            layer=dict(predictor_hidden_dims=[64, 32], target_hidden_dims=[48, 32], num_outputs=5))


def _runner(tmp=None, rnd=None, seed=31, exact=False, save_interval=50, mirror_loss_coef=None):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(N), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4                 # 400-step episodes: resets (and time-outs) inside the rollouts
    train_cfg.runner.num_steps_per_env = T
    train_cfg.runner.save_interval = save_interval
    train_cfg.algorithm.num_learning_epochs, train_cfg.algorithm.num_mini_batches = 2, 2
    if exact:
        train_cfg.runner.exact_resume = True
    if rnd is not None:
        train_cfg.algorithm.rnd_cfg = rnd
    if mirror_loss_coef is not None:      # the mirror loss WITHOUT the augmentation: the one form of symmetry RND accepts
        train_cfg.algorithm.symmetry, train_cfg.algorithm.mirror_loss_coef = False, mirror_loss_coef
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    assert (runner.alg._rnd is not None) == (rnd is not None) and PPO.rnd is None
    return runner


def _policy_state(runner):
    torch.cuda.synchronize()
    net = runner.alg.net
    return [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(),
            runner.alg.storage.rewards.clone(), runner.alg.storage._obs_all[0].clone()]


def _rnd_state(runner):
    torch.cuda.synchronize()
    rnd = runner.alg._rnd
    p, t = rnd.nets
    out = [p.params.clone(), p.adam_m.clone(), p.adam_v.clone(), p.opt_state.clone(), t.params.clone(), rnd.block.clone()]
    if rnd.norm is not None:
        out += [rnd.norm[k].clone() for k in ("mean", "var", "count", "m", "s")]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _rollout(r):
    """One stepwise rollout on the PLAIN path -- the env's own output tensors, nothing bound to the storage's slots, so the storage's
    slot T is never written -- ; -> (the bootstrap critic observation, the last observations, clones of the privileged and plain
    observations behind every step: the NEXT state of every transition as the env produced it)."""
    env, alg = r.env, r.alg
    nxt_priv, nxt_obs = [], []
    with torch.inference_mode():
        obs, priv = env.get_observations(), env.get_privileged_observations()
        for _ in range(T):
            obs, priv, rew, dones, infos = env.step(alg.act(obs, priv))
            alg.process_env_step(rew, dones, infos)
            nxt_priv.append(priv.clone())
            nxt_obs.append(obs.clone())
    return priv, obs, torch.stack(nxt_priv), torch.stack(nxt_obs)


@pytest.mark.parametrize("path", list(NETS))
def test_weight_zero_leaves_the_policy_alone(path):
    a = _runner(rnd=dict(weight=0.0, **NETS[path]))
    p0 = a.alg._rnd.nets[0].params.clone()
    t0 = a.alg._rnd.nets[1].params.clone()
    assert (a.alg._rnd.nets[0].shadow_ld(0) > 0) == (path == "fused")
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    b = _runner(rnd=None)
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert _same(_policy_state(a), _policy_state(b))
    p1 = a.alg._rnd.nets[0].params
    K = a.alg._rnd.num_outputs
    assert not torch.equal(p0[K:], p1[K:]) and torch.equal(t0, a.alg._rnd.nets[1].params)      # the predictor moved, the target did not
    assert torch.equal(p0[:K], p1[:K])                                                          # (its unused sigma slots did not either)
    log = a.alg._rnd.read_log(a.alg._log.split(a.alg.log_block().cpu()))
    print(log)
    assert np.isfinite(log["Loss/rnd"]) and log["Loss/rnd"] > 0 and log["Rnd/weight"] == 0.0 and log["Rnd/intrinsic_reward"] == 0.0
    assert float(a.alg._rnd.block[R.COUNTER]) == 3 * T and float(a.alg._rnd.nets[0].opt_state[L.OPT_STEP]) == 3 * 4
    assert float((a.alg.storage.rnd_error > 0).float().mean()) == 1.0 and not bool(a.alg.storage.rnd_intrinsic.any())


@pytest.mark.parametrize("path", list(NETS))
def test_rewards_are_extrinsic_plus_the_restated_intrinsic(path):
    r = _runner(rnd=dict(weight=0.5, gamma=0.9, **NETS[path]))
    alg, st, rnd = r.alg, r.alg.storage, r.alg._rnd
    priv, _, nxt_priv, _ = _rollout(r)
    extrinsic = st.rewards.clone()
    assert priv.data_ptr() != st._priv_all[T].data_ptr() and not alg._slot_T_written and not bool(st._priv_all[T].any())
    with torch.inference_mode():
        alg.compute_returns(priv)
    torch.cuda.synchronize()
    K, S = rnd.num_outputs, rnd.num_states
    assert (rnd.source, rnd.start, rnd.stop) == ("critic_obs", 146, 219) and S == 73
    assert torch.equal(st.rnd_states[:T], st._priv_all[:T, :, 146:219])
    # the state behind every transition is what the ENV produced: row T comes from the bootstrap observation, which the plain path never
    # puts into the storage
    assert torch.equal(st.rnd_states[1:], nxt_priv[:, :, 146:219]) and torch.equal(st.rnd_states[T], priv[:, 146:219])
    assert bool(st.rnd_states[T].any())
    rows = nxt_priv[:, :, 146:219].contiguous().flatten(0, 1)      # the expectation is built from the env's observations, not the storage's copy
    fw = lambda net: torch.cat([net.forward(0, rows[m0:m0 + 64].contiguous()) for m0 in range(0, T * N, 64)]).view(T, N, K).cpu().numpy()
    pred, target = fw(rnd.nets[0]), fw(rnd.nets[1])
    exact = R.exact_error(pred, target)
    got = st.rnd_error.cpu().numpy()
    worst = float(np.max(np.abs(got - exact) / exact))
    print("rnd_error against the restatement of forward(): rel %.3e (bar %.3e)" % (worst, R.err_bound(K)))
    assert worst <= R.err_bound(K)
    ref = R.reference(None, None, None, R.fresh_state(N), gamma=0.9, err=got, schedule=R.CONSTANT, w0=0.5)
    block = rnd.block.cpu().numpy()
    assert abs(block[R.VAR] - ref["state"]["var"]) <= 1e-10 * ref["state"]["var"] and abs(block[R.MEAN] - ref["state"]["mean"]) <= 1e-10 * ref["state"]["mean"]
    scale = R.scales(T, 0, float(block[R.STD]), True, schedule=R.CONSTANT, w0=0.5)
    intr = st.rnd_intrinsic.cpu().numpy()
    assert np.array_equal(intr.view(np.uint32), (got * scale[:, None]).view(np.uint32)) and (intr > 0).all()
    want = extrinsic.view(T, N).cpu().numpy() + intr
    assert np.array_equal(st.rewards.view(T, N).cpu().numpy().view(np.uint32), want.view(np.uint32))
    log = rnd.log_from(rnd.log_tail().cpu())
    assert log["Rnd/weight"] == 0.5 and log["Rnd/std"] == float(block[R.STD])
    assert log["Rnd/intrinsic_reward"] == pytest.approx(float(intr.astype(np.float64).mean()), rel=1e-10)
    assert log["Rnd/extrinsic_reward"] == pytest.approx(float(extrinsic.double().mean()), rel=1e-9, abs=1e-12)
    # ten predictor steps on FIXED stored rows lower the MSE
    idx = torch.arange(2 * N, dtype=torch.int64, device=st.rewards.device)
    losses = []
    for _ in range(10):
        rnd.begin_update()
        rnd.train_step(st, idx)
        losses.append(float(rnd.sums[0]))
    print("predictor MSE on fixed rows:", " ".join("%.4e" % v for v in losses))
    assert float(rnd.sums[1]) == 1.0 and all(np.isfinite(losses)) and losses[-1] < losses[0]


@pytest.mark.parametrize("state_norm", [False, True])
def test_captured_update_equals_eager_update(monkeypatch, state_norm):
    cfg = dict(weight=0.5, state_normalization=state_norm, weight_schedule=dict(mode="linear", initial_step=2, final_step=10, final_value=0.1))
    monkeypatch.delenv("HGYM_GRAPH_UPDATE", raising=False)
    a = _runner(rnd=cfg)
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert a._graph is not None and a._update_graph is not None and a.alg.update_capturable()
    sa = _policy_state(a) + _rnd_state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(rnd=cfg)
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert b._update_graph is None
    assert _same(sa, _policy_state(b) + _rnd_state(b))
    assert float(a.alg._rnd.block[R.COUNTER]) == 3 * T and float(a.alg._rnd.block[R.COUNT]) == 3 * T * N
    if state_norm:
        assert float(a.alg._rnd.norm["count"]) == 3 * T * N
    key = a.alg.update_graph_key()
    off = _runner().alg.update_graph_key()
    on, no = dict(key), dict(off)      # entries are read by name
    assert [n for n, _ in key] == [n for n, _ in off] and len(on) == len(key)
    assert on["obs_norm"] is None and (on["adv_mode"], on["adv_scratch"]) == ("batch", None) and on["rnd"] is not None and no["rnd"] is None
    assert [n for n in on if type(on[n]) is not type(no[n])] == ["rnd"]


def test_checkpoints_and_exact_resume(tmp_path):
    cfg = dict(weight=0.5, state_normalization=True, **NETS["fused"])
    u = _runner(tmp_path / "u", rnd=cfg, exact=True, save_interval=1)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    path = os.path.join(u.log_dir, "model_1.pt")
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "rnd_state_dict"}
    sd = ck["rnd_state_dict"]
    assert sd["num_envs"] == N and sd["block"].numel() == R.block_doubles(N) and float(sd["block"][R.COUNTER]) == 2 * T
    assert set(sd["state_norm"]) == {"mean", "var", "count"} and float(sd["state_norm"]["count"]) == 2 * T * N
    # both mismatches are refused by name, before anything changes
    plain = _runner(tmp_path / "p")
    p0 = plain.alg.net.params.clone()
    with pytest.raises(RuntimeError, match="carries rnd_state_dict"):
        plain.load(path, env_state=False)
    assert torch.equal(p0, plain.alg.net.params)
    plain.save(str(tmp_path / "plain.pt"))
    assert set(torch.load(str(tmp_path / "plain.pt"), map_location="cpu")) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    # exact resume: 2 iterations from the checkpoint + 2 more = the uninterrupted 4
    r = _runner(tmp_path / "r", rnd=cfg, exact=True, save_interval=50)
    r0 = _rnd_state(r)
    with pytest.raises(RuntimeError, match="has no rnd_state_dict"):
        r.load(str(tmp_path / "plain.pt"), env_state=False)
    assert _same(r0, _rnd_state(r))
    r.load(path)
    assert r.current_learning_iteration == 2 and float(r.alg._rnd.block[R.COUNTER]) == 2 * T
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(_policy_state(u) + _rnd_state(u), _policy_state(r) + _rnd_state(r))


def test_state_from_obs_on_the_plain_path_needs_the_last_observations():
    """rnd_cfg.state reads "obs": compute_returns gets the critic's bootstrap observation only, so without last_obs the plain path is
    refused (its slot T is stale), and with it row T is the env's last observation; a normalised copy applies (x - m) * s to that row too."""
    r = _runner(rnd=dict(weight=0.5, state=("obs", 658, 705), state_normalization=True, **NETS["layer"]))
    alg, st, rnd = r.alg, r.alg.storage, r.alg._rnd
    priv, obs, _, nxt_obs = _rollout(r)
    with torch.inference_mode(), pytest.raises(RuntimeError, match="last_obs"):
        alg.compute_returns(priv)
    rnd.norm["m"].fill_(0.25)
    rnd.norm["s"].fill_(2.0)
    with torch.inference_mode():
        alg.compute_returns(priv, last_obs=obs)
    torch.cuda.synchronize()
    assert torch.equal(st.rnd_states[1:], (nxt_obs[:, :, 658:705] - 0.25) * 2.0) and bool(st.rnd_states[T].any())
    assert bool((st.rnd_intrinsic[T - 1] > 0).all())


def test_separate_learn_calls_replay_the_cloning_step_correctly():
    """Four learn(1) calls -- eager, capture + replay, and two replays issued after the capturing learn() has returned -- against one
    learn(4).  What the predictor's step does not train (its sigma slots, the placeholder critic) keeps its bits, its gradient entries
    are +0.0 behind the last step, and every state is that of the single call.  (hgym_bc_grad cleared its gradient vector with a
    hipMemsetAsync once; as a node of the captured update that clear left a stale pattern on exactly these later replays.)"""
    cfg = dict(weight=0.5, **NETS["fused"])
    a = _runner(rnd=cfg)
    p = a.alg._rnd.nets[0]
    K, c0 = a.alg._rnd.num_outputs, p.bucket_split
    base = p.params.clone()
    for it in range(4):
        a.learn(num_learning_iterations=1, init_at_random_ep_len=(it == 0))
        torch.cuda.synchronize()
        assert (a._update_graph is not None) == (it >= 1)
        g = p.grads_ext
        assert not bool(g[:K].any()) and not bool(g[c0:].any()), "learn() call %d: gradient entries outside the predictor are not zero" % it
        assert torch.equal(p.params[:K], base[:K]) and torch.equal(p.params[c0:], base[c0:]), "learn() call %d" % it
    assert not torch.equal(p.params[K:c0], base[K:c0])
    b = _runner(rnd=cfg)
    b.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    assert _same(_policy_state(a) + _rnd_state(a), _policy_state(b) + _rnd_state(b))


def test_mirror_loss_and_rnd_share_the_log_block():
    """The mirror loss (no augmentation) together with RND: both tails lie behind opt_state and each reader finds its own by name."""
    r = _runner(rnd=dict(weight=0.5, **NETS["fused"]), mirror_loss_coef=0.5)
    alg = r.alg
    assert alg._mirror_loss.coef == 0.5 and alg._augment is False and alg._rnd is not None and alg._smooth is None
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    block = alg.log_block().cpu()
    assert block.numel() == alg._log.numel() == L.OPT_STATE + 2 + alg._rnd.LOG_DOUBLES
    parts = alg._log.split(block)
    assert list(parts) == ["opt", "mirror", "rnd_sums", "rnd_block"]
    assert torch.equal(parts["opt"], alg.net.opt_state.cpu()) and torch.equal(parts["mirror"], alg._mirror_loss.sums.cpu())
    mirror, rnd = alg._mirror_loss.read_log(parts), alg._rnd.read_log(parts)
    print("Loss/mirror %.4e" % mirror, rnd)
    assert np.isfinite(mirror) and mirror > 0
    assert set(rnd) == {"Loss/rnd", "Rnd/intrinsic_reward", "Rnd/extrinsic_reward", "Rnd/weight", "Rnd/std"}
    assert all(np.isfinite(v) for v in rnd.values()) and rnd["Loss/rnd"] > 0 and rnd["Rnd/intrinsic_reward"] > 0 and rnd["Rnd/weight"] == 0.5
    assert alg._smooth is None and "smooth" not in parts


def test_off_means_absent():
    r = _runner()
    alg, st = r.alg, r.alg.storage
    assert alg._rnd is None and alg.rnd is None and alg._options == () and list(alg._log.split(alg.log_block().cpu())) == ["opt"]
    assert not any(hasattr(st, k) for k in ("rnd_states", "rnd_target", "rnd_pred", "rnd_error", "rnd_intrinsic"))
    assert alg.log_block().numel() == alg.net.opt_state.numel() == L.OPT_STATE
    import hgym
    assert [v for v in vars(alg).values() if isinstance(v, hgym.NetBuffers)] == [alg.net]


def test_init_storage_refusals():
    from humanoid.algo import PPO, RandomNetworkDistillation
    from humanoid.utils.symmetry import xbot_l_mirror
    r = _runner()
    ac = r.alg.actor_critic
    alg = PPO(ac, num_mini_batches=2, device=r.device)
    alg.rnd = RandomNetworkDistillation(705, 219, dict(weight=1.0), critic_frame=73)
    alg.symmetry = xbot_l_mirror(r.env.cfg)
    with pytest.raises(ValueError, match="symmetry_augmentation"):
        alg.init_storage(N, T, [705], [219], [12])
