"""-m gpu: the mirror loss without augmentation beside the smoothness regulariser through the drop-in stack (PPO.mirror_loss_coef with
PPO.smoothness, OnPolicyRunner's mirror_loss_coef + smoothness_cfg), at 64 envs, rollouts of 8 steps, 2 minibatches
x 2 epochs -- tests/test_smoothness_runner_gpu.py's sizes.

  * init_storage with both options builds; augmentation beside the regulariser is still refused; a noise_std that tells left from right
    is refused by the column's number;
  * the captured update replays what the eager update does, bit for bit over 3 iterations; all three Loss/* values are finite and
    positive and logged;
  * learn(2) + learn(2) is learn(4); an exact resume from the middle continues bit for bit;
  * off means absent: with either option off the launches are that option's own, hgym_ppo_grad_smooth_mirror is never called;
  * with RND and per-minibatch advantages on as well the run is finite, captured equals eager, and everything logs;
  * twenty Adam steps on the three terms alone (advantages 0, value and entropy coefficients 0) lower their weighted sum, measured in
    float64 from the parameters before and after."""
import copy
import os

import numpy as np
import pytest
import torch

import mirror_smooth_common as MS
import update_options_common as U
import test_update_options_gpu as G
from hgym import _lib as L

pytestmark = pytest.mark.gpu
TASK, N, T = "humanoid_ppo", 64, 8
BOTH = dict(temporal_coef=2.0, spatial_coef=4.0)
COEF = 0.5


def _runner(tmp=None, smooth=BOTH, coef=COEF, seed=31, exact=False, save_interval=50, more=False):
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
    if smooth is not None:
        train_cfg.algorithm.smoothness_cfg = dict(smooth)
    if coef:
        train_cfg.algorithm.mirror_loss_coef = coef      # (no `symmetry`: the tables without the augmentation)
    if more:
        train_cfg.algorithm.rnd_cfg = dict(weight=0.5, predictor_hidden_dims=[256, 128, 128], target_hidden_dims=[256, 128, 128])
        train_cfg.algorithm.advantage_normalization = "minibatch"
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name=TASK, args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    alg = runner.alg
    assert (alg._smooth is not None) == (smooth is not None) and (alg._mirror_loss is not None) == bool(coef) and not alg._augment
    assert PPO.smoothness is None and PPO.mirror_loss_coef == 0.0
    return runner


def _state(runner):
    torch.cuda.synchronize()
    alg = runner.alg
    net, st = alg.net, alg.storage
    out = [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(), st._obs_all[0].clone()]
    if alg._smooth is not None:
        out += [alg._smooth.sums.clone(), alg._smooth.next_weight.clone()]
    if alg._mirror_loss is not None:
        out += [alg._mirror_loss.sums.clone()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _bare(r, **attrs):
    from humanoid.algo import PPO
    alg = PPO(r.alg.actor_critic, num_mini_batches=2, device=r.device)
    for k, v in attrs.items():
        setattr(alg, k, v)
    return alg


def test_init_storage_builds_and_its_refusals():
    from humanoid.algo.ppo import smoothness as SM
    from humanoid.utils.symmetry import xbot_l_mirror
    r = _runner()
    alg = r.alg
    assert alg._smooth.head_partials is not None and alg._smooth.head_partials.numel() == 4 * ((N * T // 2 + 63) // 64)
    assert alg._smooth.head_partials.data_ptr() % 16 == 0
    assert [type(o).__name__ for o in alg._options] == ["MirrorLoss", "Smoothness"]
    assert dict(alg.update_graph_key())["smoothness"][-1] == alg._smooth.head_partials.data_ptr()
    spec = xbot_l_mirror(r.env.cfg)
    noise = SM.env_noise_std(r.env.cfg, r.env.noise_scale_vec, 705)
    ok = _bare(r, symmetry=spec, symmetry_augmentation=False, mirror_loss_coef=COEF, smoothness=dict(BOTH, noise_std=noise))
    ok.init_storage(N, T, [705], [219], [12])      # (before the combination: ValueError)
    assert ok._smooth.head_partials is not None and ok._mirror_loss is not None
    aug = _bare(r, symmetry=spec, symmetry_augmentation=True, mirror_loss_coef=COEF, smoothness=dict(BOTH, noise_std=noise))
    with pytest.raises(ValueError, match="symmetry"):
        aug.init_storage(N, T, [705], [219], [12])
    bad = list(noise)
    c = 47 * 2 + 5 + 12 + 1      # frame 2, joint velocity 1
    bad[c] += 0.25
    lop = _bare(r, symmetry=spec, symmetry_augmentation=False, mirror_loss_coef=COEF, smoothness=dict(BOTH, noise_std=bad))
    with pytest.raises(ValueError, match="column %d " % c):
        lop.init_storage(N, T, [705], [219], [12])
    lop.smoothness = dict(temporal_coef=2.0, noise_std=bad)      # the spatial term off: the noise is not looked at
    lop.init_storage(N, T, [705], [219], [12])
    two = _bare(r, symmetry=spec, symmetry_augmentation=False, mirror_loss_coef=COEF, smoothness=dict(BOTH, noise_std=noise))
    two._world = 2
    with pytest.raises(ValueError, match="one rank"):
        two.init_storage(N, T, [705], [219], [12])


def test_captured_update_equals_eager_update_and_the_losses_are_logged(monkeypatch, tmp_path):
    for k in ("HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_GRAPH", "HGYM_ASYNC", "HGYM_ROLLOUT_CRITIC", "HGYM_LOG_SINK"):
        monkeypatch.delenv(k, raising=False)
    a = _runner(tmp_path / "a")
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    a.wait_for_saves()
    sa = _state(a)
    assert a._update_graph is not None and a.alg.update_capturable()
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(tmp_path / "b")
    calls = []
    both = b.alg.net.ppo_grad_smooth_mirror
    monkeypatch.setattr(b.alg.net, "ppo_grad_smooth_mirror", lambda *x: (calls.append("both"), both(*x)))
    monkeypatch.setattr(b.alg.net, "ppo_grad_smooth", lambda *x: calls.append("smooth"))
    monkeypatch.setattr(b.alg.net, "ppo_grad", lambda *x: calls.append("plain"))
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    b.wait_for_saves()
    assert b._update_graph is None and calls == ["both"] * (3 * 2 * 2)
    assert _same(sa, _state(b)), "the captured update and the eager one differ"
    assert all(torch.isfinite(t.double()).all() for t in sa)
    o = b.alg.read_log(b.alg.log_block().cpu())
    scalars = dict(b.alg.log_scalars())
    print("Loss/mirror %.4e Loss/smooth_temporal %.4e Loss/smooth_spatial %.4e valid_fraction %.3f" %
          (scalars["Loss/mirror"], scalars["Loss/smooth_temporal"], scalars["Loss/smooth_spatial"], b.alg.last_smoothness["valid_fraction"]))
    assert list(scalars) == ["Loss/mirror", "Loss/smooth_temporal", "Loss/smooth_spatial"]
    assert all(np.isfinite(v) and v > 0 for v in scalars.values()) and np.isfinite(o["mean_value_loss"])
    assert 0.5 < b.alg.last_smoothness["valid_fraction"] <= 1.0 and b.alg.last_mirror_loss == scalars["Loss/mirror"]
    assert list(b.alg._log.split(b.alg.log_block().cpu())) == ["opt", "mirror", "smooth"]
    key = a.alg.update_graph_key()
    alone = _runner(coef=0.0).alg.update_graph_key()
    assert [n for n, _ in alone] == [n for n, _ in key] and len(dict(alone)["smoothness"]) + 1 == len(dict(key)["smoothness"])


def test_loss_keys_reach_the_writer(monkeypatch, tmp_path):
    seen = {}
    r = _runner(tmp_path / "log")
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)      # opens the writer
    r.wait_for_saves()
    if r.writer is not None:
        monkeypatch.setattr(r.writer, "add_scalar", lambda k, v, it: seen.setdefault(k, []).append(float(v)))
    r.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    r.wait_for_saves()
    torch.cuda.synchronize()
    assert r.alg.last_smoothness is not None and r.alg.last_mirror_loss is not None
    if r.writer is not None:
        for k in ("Loss/mirror", "Loss/smooth_temporal", "Loss/smooth_spatial"):
            assert k in seen and all(np.isfinite(v) and v > 0 for v in seen[k]), (k, seen.get(k))


def test_two_and_two_is_four(monkeypatch):
    monkeypatch.delenv("HGYM_GRAPH_UPDATE", raising=False)
    a = _runner()
    a.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    a.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    b = _runner()
    b.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    assert _same(_state(a), _state(b))


def test_exact_resume_from_the_middle(tmp_path, monkeypatch):
    monkeypatch.delenv("HGYM_GRAPH_UPDATE", raising=False)
    u = _runner(tmp_path / "u", exact=True, save_interval=1)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    r = _runner(tmp_path / "r", exact=True, save_interval=50)
    r.load(os.path.join(u.log_dir, "model_1.pt"))
    assert r.current_learning_iteration == 2
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(_state(u), _state(r))


@pytest.mark.parametrize("off", ["mirror", "smooth"])
def test_off_means_absent(monkeypatch, off):
    """With either option off the other's own entry point runs, as before the combination: the new one is never called."""
    r = _runner(coef=0.0) if off == "mirror" else _runner(smooth=None)
    alg = r.alg
    assert (alg._smooth is None or alg._smooth.head_partials is None)
    calls = []
    monkeypatch.setattr(alg.net, "ppo_grad_smooth_mirror", lambda *a: calls.append("both"))
    for name in ("ppo_grad", "ppo_grad_smooth"):
        fn = getattr(alg.net, name)
        monkeypatch.setattr(alg.net, name, lambda *a, fn=fn, name=name: (calls.append(name), fn(*a)))
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert calls == ["ppo_grad_smooth" if off == "mirror" else "ppo_grad"] * (2 * 2 * 2)
    names = list(alg._log.split(alg.log_block().cpu()))
    assert names == (["opt", "smooth"] if off == "mirror" else ["opt", "mirror"])


def test_with_rnd_and_minibatch_advantages(monkeypatch):
    monkeypatch.delenv("HGYM_GRAPH_UPDATE", raising=False)
    a = _runner(more=True)
    assert a.alg._rnd is not None and a.alg._adv_mode == "minibatch"
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    sa = _state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(more=True)
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert _same(sa, _state(b)) and all(torch.isfinite(t.double()).all() for t in sa)
    block = b.alg.log_block().cpu()
    parts = b.alg._log.split(block)
    b.alg.read_log(block)
    scalars = dict(b.alg.log_scalars())
    assert list(parts)[:2] == ["opt", "mirror"] and "smooth" in parts
    for k in ("Loss/mirror", "Loss/smooth_temporal", "Loss/smooth_spatial", "Loss/rnd"):
        assert np.isfinite(scalars[k]) and scalars[k] > 0, (k, scalars)
    assert block.numel() == L.OPT_STATE + 2 + b.alg._rnd.LOG_DOUBLES + 4


# ---------------------------------------------------------------------------------------------- the three terms fall together
def test_twenty_steps_on_the_three_terms_alone_lower_their_weighted_sum():
    """Advantages 0, value and entropy coefficients 0, a fixed small learning rate (tests/test_smoothness_runner_gpu.py gives the reason for
    1e-5): twenty Adam steps of hgym_ppo_grad_smooth_mirror.  c_m mse_m + lamT mse_T + lamS mse_S is measured in plain torch float64 from the
    net's parameters before and after, the spatial targets on the perturbed rows the device wrote in the first step."""
    import test_mirror_smooth_gpu as TG
    opts = U.Options("bf16-fused", None, "scalar", False, False, False, True)
    base = MS.case_of(opts)
    cols = list(base["cols"])
    cols[4] = torch.zeros_like(cols[4])
    case = dict(base, cols=cols, ppo=dict(base["ppo"], value_coef=0.0, entropy_coef=0.0))
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case, value_loss_coef=0.0, entropy_coef=0.0, adaptive=False, mirror_coef=MS.COEF)
    net.opt_state[L.OPT_LR] = 1e-5
    obs, idx = case["cols"][0], case["idx"]
    src, sign = torch.tensor(case["spec"].act_src), torch.tensor(case["spec"].act_sign, dtype=torch.float64)
    w = case["weight"].double()
    near = None

    def total():
        params = {k: v.cpu() for k, v in net.state_dict().items()}
        priv = torch.zeros(len(idx), U.SHAPES[opts.path]["net"][1])
        mu = lambda rows: U.forward(opts, params, case["stats"], rows, priv)[0]
        m = mu(obs[idx])
        se_m = ((m - sign * mu(obs[case["pair"]])[:, src]) ** 2).sum()
        se_t = (w[:, None] * (m - mu(obs[case["nxt"]])) ** 2).sum()
        se_s = ((m - mu(near)) ** 2).sum()
        return float(MS.COEF * se_m + MS.LAM_T * se_t + MS.LAM_S * se_s) / m.numel()
    for step in range(20):
        r = TG._call(net, opts, case, ppo, True, "both")
        if step == 0:
            near = r["pr"][:case["B"], :obs.shape[1]].cpu().clone()
            before = total()
        net.ppo_apply(ppo)
    torch.cuda.synchronize()
    after = total()
    print("c_m mse_m + lamT mse_T + lamS mse_S: %.6e -> %.6e after 20 Adam steps on the three terms alone" % (before, after))
    assert np.isfinite(after) and after < before
