"""-m gpu: empirical observation normalisation through the drop-in stack (ActorCritic(empirical_normalization=True), PPO,
OnPolicyRunner), at 64 envs and rollouts of 6 steps.

  * one iteration by hand: the statistics are frozen until the update has run (the minibatch that follows the rollout sees ratio 1), and
    end up as the float64 merge of the rollout's raw rows, within the bounds of tests/obs_norm_common.py;
  * the captured update replays what the eager update does, normaliser step included;
  * checkpoints carry the statistics on both writer paths; load() restores them, refuses both mismatches, and an exact resume continues
    the run bit for bit;
  * the exported policy takes raw observations;
  * an identity normaliser (eps = 0, until = 0) leaves the fused rollout and the fused evaluation bit for bit what they are without it, and
    under planted power-of-two scales the fused rollout's stored outputs are the policy launch's on the stored raw rows;
  * two ranks end with one state."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import obs_norm_common as ON
from hgym import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK, N, T = "humanoid_ppo", 64, 6
NORM_KEYS = ("obs_norm_state_dict", "critic_obs_norm_state_dict")


def _runner(tmp=None, norm=True, seed=31, precision="bf16", exact=False, save_interval=2, policy=None, runner_place=False, epochs=None,
            minibatches=None, dev=None):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = precision
    argv = ["--task=" + TASK, "--headless", "--num_envs", str(N), "--seed", str(seed)]
    if dev:
        argv += ["--sim_device", dev, "--rl_device", dev]
    args = get_args(argv)
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4                 # 400-step episodes: resets inside the rollouts
    train_cfg.runner.num_steps_per_env = T
    train_cfg.runner.save_interval = save_interval
    if exact:
        train_cfg.runner.exact_resume = True
    if epochs is not None:
        train_cfg.algorithm.num_learning_epochs, train_cfg.algorithm.num_mini_batches = epochs, minibatches
    if norm:
        if runner_place:
            train_cfg.runner.empirical_normalization = True      # rsl_rl's place
        else:
            train_cfg.policy.empirical_normalization = True
        for k, v in (policy or {}).items():
            setattr(train_cfg.policy, k, v)
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    assert runner.alg.actor_critic.empirical_normalization == norm and (runner.alg.net.obs_norm is not None) == norm
    return runner


def _stats(runner):
    torch.cuda.synchronize()
    net = runner.alg.net
    return [net.norm_view(n, k).clone() for k in (0, 1) for n in ("mean", "var", "mean_f", "scale_f", "bias")] + [net.norm_view("header").clone()]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _run_state(runner):
    torch.cuda.synchronize()
    net = runner.alg.net
    return [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(),
            runner.alg.storage._obs_all[0].clone()] + (_stats(runner) if net.obs_norm is not None else [])


def test_one_iteration_by_hand():
    """rollout -> clone the raw rows -> compute_returns -> update (one epoch, one minibatch).  The update differentiates the net the
    rollout ran: its only minibatch sees ratio 1 -- the surrogate is -mean(normalised advantages) = 0 and the KL of the policy with
    itself is the 12 log(1 + 1e-5) of the learning-rate rule's expression -- because the statistics move only at the END of update().
    Had they moved before it (identity -> the rollout's statistics: scales of 10 .. 100 on the near-constant columns), the ratios would be
    nowhere near 1.  Afterwards the state is the float64 merge of the T N raw rows, count T N, and the rows in the storage are still raw."""
    r = _runner(runner_place=True, epochs=1, minibatches=1)
    env, alg, net = r.env, r.alg, r.alg.net
    before = _stats(r)
    assert float(net.norm_view("header")[2]) == 0.0 and alg._ppo_cfg.grad_norm_ready == 0 and alg._obs_norm == (1e-2, None)
    with torch.inference_mode():
        obs, priv = env.get_observations(), env.get_privileged_observations()
        for _ in range(T):
            obs, priv, rew, dones, infos = env.step(alg.act(obs, priv))
            alg.process_env_step(rew, dones, infos)
        rows = [alg.storage._obs_all[:T].flatten(0, 1).clone(), alg.storage._priv_all[:T].flatten(0, 1).clone()]
        assert _same(before, _stats(r)), "the statistics moved during the rollout"
        alg.compute_returns(priv)
    alg.update()
    torch.cuda.synchronize()
    opt = net.opt_state.cpu()
    assert float(opt[L.OPT_MINIBATCHES]) == 1.0 and float(opt[L.OPT_STEP]) == 1.0
    print("surrogate %.3e  KL %.3e" % (float(opt[L.OPT_SURROGATE_SUM]), float(opt[L.OPT_KL_LAST])))
    # bf16 operands (1e-2 relative on mu, |mu| < 1 at initialisation, sigma = 1): KL <= 12 (1e-2)^2 / 2 + 12e-5 < 1e-3, and
    # |surrogate| = |mean(adv (ratio - 1))| <= mean|adv| max|ratio - 1| stays below 1e-2 while the log-probabilities agree to 1e-2
    assert abs(float(opt[L.OPT_SURROGATE_SUM])) < 1e-2 and 0.0 <= float(opt[L.OPT_KL_LAST]) < 1e-3
    h = net.norm_view("header").cpu()
    assert float(h[2]) == float(h[3]) == T * N
    for k, K in enumerate((705, 219)):
        x = rows[k].cpu().numpy()
        ref = ON.merge(ON.initial(K), x)
        dm, dv = ON.bounds(x)
        mean, var = net.norm_view("mean", k).cpu().numpy(), net.norm_view("var", k).cpu().numpy()
        assert np.abs(mean - ref["mean"]).max() <= dm and np.abs(var - ref["var"]).max() <= dv
        wm, ws = ON.derived(mean, var, 1e-2)
        assert np.array_equal(net.norm_view("mean_f", k).cpu().numpy(), wm)
        nz = alg.actor_critic.critic_obs_normalizer if k else alg.actor_critic.obs_normalizer
        assert nz.count == T * N and torch.equal(nz.mean.cpu(), torch.from_numpy(mean)) and torch.equal(nz.var.cpu(), torch.from_numpy(var))
        # forward(x) of the host-side module is the plain expression
        want = (x[:5].astype(np.float64) - mean) / (np.sqrt(var) + 1e-2)
        np.testing.assert_allclose(nz(rows[k][:5].double()).cpu().numpy(), want, rtol=1e-12, atol=1e-12)
    assert not _same(before, _stats(r))


def test_captured_update_equals_eager_update(monkeypatch):
    """learn(3): eager iteration, capture + replay, replay -- against HGYM_GRAPH_UPDATE=0.  The normaliser step is part of the captured
    update (same launches, same arguments every iteration): parameters, Adam state and statistics end identical."""
    monkeypatch.delenv("HGYM_GRAPH_UPDATE", raising=False)
    a = _runner()
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert a._graph is not None and a._update_graph is not None and a.alg.update_capturable()
    sa = _run_state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner()
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert b._update_graph is None
    sb = _run_state(b)
    assert float(a.alg.net.norm_view("header")[2]) == 3 * T * N
    assert _same(sa, sb)
    key_on, key_off = a.alg.update_graph_key(), _runner(norm=False).alg.update_graph_key()
    assert dict(key_on)["obs_norm"] == (1e-2, None) and dict(key_off)["obs_norm"] is None


def test_checkpoints_carry_the_statistics_and_an_exact_resume_is_the_run(tmp_path, monkeypatch):
    u = _runner(tmp_path / "u", exact=True)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    path = os.path.join(u.log_dir, "model_2.pt")
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"} | set(NORM_KEYS)
    for key, K in zip(NORM_KEYS, (705, 219)):
        e = ck[key]
        assert set(e) == {"mean", "var", "count", "eps", "until"} and e["mean"].dtype == torch.float64 and e["mean"].shape == (K,)
        assert e["count"] == 3 * T * N and e["eps"] == 1e-2 and e["until"] is None and bool((e["var"] >= 0).all())
    # the blocking writer writes the same entries as the background one
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "0")
    u.save(str(tmp_path / "sync.pt"))
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "1")
    u.save(str(tmp_path / "async.pt"))
    s, a = (torch.load(str(tmp_path / n), map_location="cpu") for n in ("sync.pt", "async.pt"))
    assert set(s) == set(a) == set(ck)
    for key in NORM_KEYS:
        assert torch.equal(s[key]["mean"], a[key]["mean"]) and torch.equal(s[key]["var"], a[key]["var"])
        assert {k: v for k, v in s[key].items() if k not in ("mean", "var")} == {k: v for k, v in a[key].items() if k not in ("mean", "var")}
        assert s[key]["count"] == 4 * T * N
    # load into a fresh runner: the same function of raw observations, bit for bit
    f = _runner(None, exact=False, seed=77)
    f.load(str(tmp_path / "async.pt"), env_state=False)
    rows = u.alg.storage._obs_all[1].clone()
    assert _same(_stats(f), _stats(u))
    assert torch.equal(f.alg.actor_critic.act_inference(rows), u.alg.actor_critic.act_inference(rows))
    assert torch.equal(f.alg.actor_critic.evaluate(u.alg.storage._priv_all[1]), u.alg.actor_critic.evaluate(u.alg.storage._priv_all[1]))
    # both mismatches are refused, naming the key, before the parameters change
    plain = _runner(tmp_path / "p", norm=False)
    p0 = plain.alg.net.params.clone()
    with pytest.raises(RuntimeError, match="obs_norm_state_dict"):
        plain.load(str(tmp_path / "async.pt"), env_state=False)
    assert torch.equal(plain.alg.net.params, p0)
    plain.save(str(tmp_path / "plain.pt"))
    assert set(torch.load(str(tmp_path / "plain.pt"), map_location="cpu")) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    f0 = _run_state(f)
    with pytest.raises(RuntimeError, match="obs_norm_state_dict"):
        f.load(str(tmp_path / "plain.pt"), env_state=False)
    assert _same(f0, _run_state(f))
    # exact resume: a fresh env + runner continue from model_2.pt (3 iterations done) for one iteration = the uninterrupted run's fourth
    r = _runner(tmp_path / "r", exact=True)
    r.load(path)
    assert r.current_learning_iteration == 3 and float(r.alg.net.norm_view("header")[2]) == 3 * T * N
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(_run_state(u), _run_state(r))


def test_exported_policy_takes_raw_observations(tmp_path):
    """An fp32 run, two iterations (the statistics are the rollouts'): policy_1.pt -- the same nn.Sequential, its first layer folded --
    on raw CPU rows against act_inference on the device, at the fp32 bar of tests/test_net_gpu.py; so does get_inference_policy("cpu")."""
    from humanoid.utils import export_policy_as_jit
    r = _runner(precision="f32")
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    ac = r.alg.actor_critic
    assert float(ac.obs_normalizer.var.min()) < 0.5 and ac.obs_normalizer.count == 2 * T * N
    rows = r.alg.storage._obs_all[2].clone()
    want = ac.act_inference(rows).cpu().double()
    export_policy_as_jit(ac, str(tmp_path))
    pol = torch.jit.load(str(tmp_path / "policy_1.pt"))
    for what, got in (("policy_1.pt", pol(rows.cpu())), ("get_inference_policy(cpu)", r.get_inference_policy(device="cpu")(rows.cpu()))):
        err = float((got.detach().double() - want).abs().max() / want.abs().max())
        print("%s vs act_inference: %.3e" % (what, err))
        assert err <= 1e-5, (what, err)
    # without the fold the same module is another function: the check above is not vacuous
    raw = copy.deepcopy(ac.actor).cpu()(rows.cpu()).detach().double()
    assert float((raw - want).abs().max() / want.abs().max()) > 1e-2


def test_identity_normaliser_leaves_fused_rollout_and_evaluation_bit_identical():
    """eps = 0, until = 0: mean 0, scale 1, never merged.  The one-launch rollout step and the one-launch evaluation step read the first
    layer's operand copies and its bias through the same two places as every other kernel: with the identity fold they compute, bit for
    bit, what they compute without the block."""
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    runs = []
    for norm in (False, True):
        r = _runner(norm=norm, policy=dict(normalization_eps=0.0, normalization_until=0), seed=41)
        assert r.env.rollout_fused_mode(r.alg.net) == "inline"
        args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(N), "--seed", "43"])
        env_cfg = copy.deepcopy(task_registry.get_cfgs(name=TASK)[0])
        env_cfg.seed = 43
        eval_env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
        assert eval_env.eval_rollout_supported(r.alg.net)
        ev = r.evaluate(eval_env, 8, fused=True)
        r.learn(num_learning_iterations=1, init_at_random_ep_len=False)      # (the update does not touch the columns compared below)
        torch.cuda.synchronize()
        st = r.alg.storage
        runs.append((ev, [t.clone() for t in (st._obs_all[1:], st._priv_all[1:], st.actions, st.mu, st.sigma, st.actions_log_prob, st.values, st.rewards)]))
        if norm:
            assert float(r.alg.net.norm_view("header")[2]) == 0.0
    (ev0, c0), (ev1, c1) = runs
    assert {k: v for k, v in ev0.items() if v == v} == {k: v for k, v in ev1.items() if v == v} and ev0.keys() == ev1.keys()
    assert _same(c0, c1)


def test_fused_rollout_reads_the_scaled_operand_copies():
    """The env produces the rows, so a rollout cannot be fed scaled rows -- but its stored outputs can be held against the policy launch.
    Planted statistics mean 0, var 4^k (k in -2 .. 2 per column), eps = 0, until = 0 (never merged): scales 2^-k.  After a one-launch-a-step
    rollout, the stored mu and values of a slot equal, bit for bit, hgym_policy_act of the normalised net on the slot's stored raw rows AND
    hgym_policy_act of a plain net with the same parameters on those rows times 2^-k: the rollout launch read the scaled operand copies."""
    from hgym import NetBuffers
    r = _runner(policy=dict(normalization_eps=0.0, normalization_until=0), seed=45)
    net, st = r.alg.net, r.alg.storage
    ks = [(torch.arange(K) % 5 - 2).double() for K in (705, 219)]
    net.load_norm_state(dict(obs=dict(mean=torch.zeros(705, dtype=torch.float64), var=4.0 ** ks[0], count=0.0),
                             critic_obs=dict(mean=torch.zeros(219, dtype=torch.float64), var=4.0 ** ks[1], count=0.0)))
    sf = [net.norm_view("scale_f", k).clone() for k in (0, 1)]
    assert torch.equal(sf[0].cpu(), (2.0 ** -ks[0]).float()) and torch.equal(sf[1].cpu(), (2.0 ** -ks[1]).float())
    assert r.env.rollout_fused_mode(net) == "inline"
    params0, stats0 = net.params.clone(), _stats(r)
    r.learn(num_learning_iterations=1, init_at_random_ep_len=False)
    torch.cuda.synchronize()
    assert not torch.equal(net.params, params0)
    net.params.copy_(params0)           # the parameters the rollout ran
    net.sync_shadow()
    assert _same(stats0, _stats(r))     # until = 0: the update's normaliser step merged nothing
    plain = NetBuffers(net.cfg, "cuda")
    plain.params.copy_(params0)
    plain.sync_shadow()
    z = torch.zeros(N, 12, device="cuda")
    for t in (1, T - 1):                # (slot 0 was overwritten by the update's clear())
        x, xp = st._obs_all[t].clone(), st._priv_all[t].clone()
        oa = net.act(x, xp, z=z)
        ob = plain.act((x * sf[0]).contiguous(), (xp * sf[1]).contiguous(), z=z)
        torch.cuda.synchronize()
        assert float(st.mu[t].abs().max()) > 0
        for got in (oa, ob):
            assert torch.equal(st.mu[t].view(torch.int32), got["mu"].view(torch.int32)), t
            assert torch.equal(st.values[t].reshape(-1).view(torch.int32), got["values"].reshape(-1).view(torch.int32)), t
    # and it is not vacuous: without the scale the same rows give another mu
    assert not torch.equal(plain.act(st._obs_all[1].clone(), st._priv_all[1].clone(), z=z)["mu"], st.mu[1])


def _rank(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "humanoid-gym_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["HGYM_COMM"] = "rccl"        # the collective exchange (gloo here); the normaliser's sums use a collective in any case
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = _runner(seed=5 + rank, dev="cuda:0")
    assert r.alg._world == world and not r.alg.update_capturable()
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    net = r.alg.net
    torch.save(dict(params=net.params.cpu(), stats=[t.cpu() for t in _stats(r)], obs=r.alg.storage._obs_all[1].cpu(),
                    update_graph=r._update_graph is not None), os.path.join(out_dir, "n%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_end_with_one_state(tmp_path):
    """Two ranks share the GPU over gloo, each with its own 64 envs, two iterations: the raw sums pass through one all-reduce before
    the merge, so both ranks hold the same statistics (count = both shards, both iterations) and the same parameters."""
    port = 31300 + (os.getpid() % 2000)
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(os.path.join(str(tmp_path), "n%d.pt" % i)) for i in range(2))
    assert not torch.equal(a["obs"], b["obs"])                    # different env shards
    assert torch.equal(a["params"], b["params"]) and torch.isfinite(a["params"]).all()
    assert _same(a["stats"], b["stats"])
    hdr = a["stats"][-1]
    assert float(hdr[2]) == float(hdr[3]) == 2 * T * N * 2
    assert not a["update_graph"] and not b["update_graph"]
