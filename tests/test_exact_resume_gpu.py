"""-m gpu: a restored env IS the env, and a resumed run IS the run (LeggedRobot.state_dict / load_state_dict, the envstate_<it>.pt
sidecar of OnPolicyRunner.save / load).  Every comparison is torch.equal: the claim is bit-identity.

  * the env alone on the stepwise path: XBot-L defaults, the generic options (trimesh terrain, both curricula, height measurements)
    and a task with `_reward_<name>` terms -- over a window that holds terminations, time-outs, command resamples and pushes;
  * reset_idx after a restore draws what the original draws;
  * a whole run: learn(4) with checkpoints every 2 iterations against a fresh env + runner that loads model_2.pt and learns 1 more,
    under the default plan (fused rollout, both HIP graphs, background writer), the eager plans, the stepwise rollout and the deferred
    critic, and across plans that are asserted bit-identical to each other elsewhere;
  * with the switch off nothing changes; synchronous and background sidecars hold the same tensors.

One figure of the env is not a function of its inputs alone: extras["episode"] (`extras_episode`) is the mean over the envs that reset in
a step, and its fp32 sum is formed by atomics in arrival order -- exact, hence the same bits in every run, only while at most two envs
reset in that step (tests/test_fused_gpu.py and tests/test_reset_idx_gpu.py compare it with a tolerance for that reason).  It feeds
logging only.  Measured here with 256 envs and 400-step episodes (several envs reset in most steps): the resumed run equalled the
uninterrupted one in every parameter, moment, counter and env tensor, and differed in the last bit of 3 of the 22 `extras_episode`
entries.  The whole-run tests therefore use 64 envs and ASSERT that the figure was formed in the exact regime (`_exact_regime`: the
last step with a reset had at most two) instead of excluding it: the state dicts are compared whole.

A restored env has the fused rollout's scratch block and first-layer partial sums of ANOTHER history (run R's env has stepped without
ever running a fused rollout; run U's has run three): the whole-run tests are the proof that a rollout's first launch reads neither."""
import copy
import os

import pytest
import torch
from hgym import _lib as L

pytestmark = pytest.mark.gpu

TASK = "humanoid_ppo"


def _cfgs(num_envs, seed, task=TASK):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=" + task, "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=task))      # (the registry hands out its singletons)
    env_cfg.seed = train_cfg.seed = seed
    return args, env_cfg, train_cfg


def _short_episodes(env_cfg):
    """dt = 0.01 s: episodes of 400 steps, commands resampled every 20, a push every 15."""
    env_cfg.env.episode_length_s = 4
    env_cfg.commands.resampling_time = 0.2
    env_cfg.domain_rand.push_interval_s = 0.15
    return env_cfg


def _generic(env_cfg):
    t = env_cfg.terrain
    t.mesh_type, t.curriculum, t.measure_heights, t.num_rows, t.num_cols, t.border_size = "trimesh", True, True, 5, 4, 5
    t.max_init_terrain_level = 2
    env_cfg.commands.curriculum = True
    return env_cfg


def _custom_task():
    from humanoid.envs import task_registry, XBotLFreeEnv, XBotLCfg, XBotLCfgPPO
    name = "exact_resume_custom"
    if name not in task_registry.task_classes:
        class TermEnv(XBotLFreeEnv):
            def _reward_alive(self):
                return torch.ones(self.num_envs, device=self.device)

            def _reward_zz_dof(self):
                return torch.sum(torch.square(self.dof_pos), dim=1)

        class TermCfg(XBotLCfg):
            class rewards(XBotLCfg.rewards):
                class scales(XBotLCfg.rewards.scales):
                    alive = 0.7
                    zz_dof = -0.02
        task_registry.register(name, TermEnv, TermCfg(), XBotLCfgPPO())
    return name


def _env(args, env_cfg):
    from humanoid.envs import task_registry
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=copy.deepcopy(env_cfg))
    return env


def _same_state(a, b, what, skip=()):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        if k == "meta" or k in skip:
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k], b[k]), "%s: `%s` differs in %d places" % (what, k, int((a[k] != b[k]).sum()))
    if "meta" not in skip:
        assert a["meta"] == b["meta"], (what, a["meta"], b["meta"])


def _record(env, out):
    obs, priv, rew, reset, extras = out
    b = env._buf
    rec = dict(obs=obs, priv=priv, rew=rew, reset=reset, time_out=env.time_out_buf, extras_time_outs=extras["time_outs"],
               extras_episode=b.extras_episode, commands=env.commands, push=env.rand_push_force, ep_len=env.episode_length_buf)
    for k, v in extras["episode"].items():
        rec["episode/" + k] = v
    if b.extras_custom is not None:
        rec["extras_custom"] = b.extras_custom
    return {k: v.clone() for k, v in rec.items()}


# ------------------------------------------------------------------------------------------------ the env alone
@pytest.mark.parametrize("variant", ["defaults", "generic", "custom_terms"])
def test_restored_env_steps_like_the_original(variant):
    """Env A: k steps, snapshot, m more steps recorded.  Env B (same config): another number of steps on other actions, the snapshot
    loaded, the same m actions.  Every output of every step and the final state are equal.  The window is not vacuous: the counts of
    terminations, time-outs, command resamples and pushes in it are asserted.  (Episode lengths are spread so that the time-outs come
    one env at a time: extras["episode"] is a mean whose fp32 sum is formed in arrival order, exact for up to two envs a step.)"""
    N, k, m, other_k = 128, 12, 48, 5
    task = _custom_task() if variant == "custom_terms" else TASK
    args, env_cfg, _ = _cfgs(N, 21, task)
    _short_episodes(env_cfg)
    if variant == "generic":
        _generic(env_cfg)
    g = torch.Generator().manual_seed(5)
    actions = (torch.randn(k + m, N, 12, generator=g) * 0.5).cuda()
    ep = (torch.arange(N) * 37) % 300
    ep[5], ep[77], ep[101] = 400 - k - 4, 400 - k - 19, 400 - k - 33          # three time-outs inside the window, on different steps

    A = _env(args, env_cfg)
    A.reset()
    A.episode_length_buf = ep.cuda()
    for t in range(k):
        A.step(actions[t])
    sd = A.state_dict()
    keep = {n: v.clone() for n, v in sd.items() if n != "meta"}
    assert sd["meta"]["num_envs"] == N and sd["meta"]["optional"]["terrain_levels"] == (variant == "generic")
    assert sd["meta"]["optional"]["custom_sums"] == (variant == "custom_terms")
    rec_a = [_record(A, A.step(actions[k + t])) for t in range(m)]
    end_a = A.state_dict()
    assert all(torch.equal(sd[n], keep[n]) for n in keep), "the snapshot is a view: stepping the env changed it"

    B = _env(args, env_cfg)
    B.reset()
    for t in range(other_k):
        B.step(actions[t] * -0.3)
    ptrs = {n: t.data_ptr() for n, t, _ in B._buf.state_entries() if t is not None}
    B.load_state_dict(sd)
    assert {n: t.data_ptr() for n, t, _ in B._buf.state_entries() if t is not None} == ptrs
    assert B.obs_buf.data_ptr() in (B._outs[0][0].data_ptr(), B._outs[1][0].data_ptr())
    _same_state(B.state_dict(), sd, variant + ": right after the load")
    rec_b = [_record(B, B.step(actions[k + t])) for t in range(m)]
    end_b = B.state_dict()
    torch.cuda.synchronize()

    for t, (ra, rb) in enumerate(zip(rec_a, rec_b)):
        assert set(ra) == set(rb)
        for name in ra:
            assert torch.equal(ra[name], rb[name]), "%s: `%s` differs at step %d after the restore" % (variant, name, t)
    _same_state(end_a, end_b, variant + ": final state")

    # what the window held
    time_outs = sum(int(r["time_out"].sum()) for r in rec_a)
    terminations = sum(int((r["reset"] & ~r["time_out"]).sum()) for r in rec_a)
    prev_cmd, prev_push, resamples, pushes = sd["state"][0:4].t(), None, 0, 0
    for r in rec_a:
        changed = (r["commands"][:, :2] != prev_cmd[:, :2]).any(dim=1) & ~r["reset"]
        resamples += int(changed.sum())
        pushes += int(prev_push is not None and not torch.equal(r["push"], prev_push))
        prev_cmd, prev_push = r["commands"], r["push"]
    print("%s: %d terminations, %d time-outs, %d command resamples, %d pushes in %d steps" % (variant, terminations, time_outs, resamples, pushes, m))
    assert time_outs >= 1 and terminations >= 1 and resamples >= 1 and pushes >= 1, (terminations, time_outs, resamples, pushes)
    if variant == "custom_terms":
        assert float(end_a["custom_sums"].abs().max()) > 0


def test_reset_idx_after_a_restore_draws_what_the_original_draws():
    """counters[3], the call number that keys reset_idx's draws, travels.  (Two ids: their extras["episode"] mean is an exact sum.)"""
    N = 64
    args, env_cfg, _ = _cfgs(N, 22)
    g = torch.Generator().manual_seed(6)
    actions = (torch.randn(8, N, 12, generator=g) * 0.5).cuda()
    A = _env(args, env_cfg)
    A.reset()
    for t in range(4):
        A.step(actions[t])
    A.reset_idx([3, 9])
    A.reset_idx([50, 9])
    sd = A.state_dict()
    assert int(sd["counters"][L.CNT_RESET_CALL]) == 2
    A.reset_idx([7, 40])
    A.step(actions[4])
    end_a = A.state_dict()
    B = _env(args, env_cfg)
    B.reset()
    B.step(actions[5])
    B.reset_idx([1])
    B.load_state_dict(sd)
    B.reset_idx([7, 40])
    B.step(actions[4])
    _same_state(B.state_dict(), end_a, "reset_idx after a restore")
    assert int(B._buf.counters[L.CNT_RESET_CALL]) == 3
    # ... and it is the call number that does it: with counters[3] put back to 0 the same call draws other joint offsets
    C_ = _env(args, env_cfg)
    C_.reset()
    C_.load_state_dict(sd)
    C_._buf.counters[L.CNT_RESET_CALL] = 0
    C_.reset_idx([7, 40])
    B.load_state_dict(sd)
    B.reset_idx([7, 40])
    torch.cuda.synchronize()
    assert not torch.equal(C_.dof_pos[7], B.dof_pos[7])


def test_refusals_on_a_live_env():
    N = 64
    args, env_cfg, _ = _cfgs(N, 23)
    env = _env(args, env_cfg)
    env.reset()
    sd = env.state_dict()
    dev = env.device
    sink = dict(values=torch.zeros(N, device=dev), rewards=torch.zeros(N, device=dev), dones=torch.zeros(N, dtype=torch.bool, device=dev),
                step=torch.zeros(1, dtype=torch.int64, device=dev), gamma=0.99)
    env.bind_transition(sink, defer_finalize=True)
    env.step(torch.zeros(N, 12, device=dev))
    with pytest.raises(ValueError, match="_pending_fin"):
        env.load_state_dict(sd)
    with pytest.raises(ValueError, match="_pending_fin"):
        env.state_dict()
    env.run_finalize(env.take_pending_finalize())
    env.bind_transition(None)
    env._in_rollout = True                # what rollout_begin leaves until rollout_end
    with pytest.raises(ValueError, match="_in_rollout"):
        env.state_dict()
    with pytest.raises(ValueError, match="_in_rollout"):
        env.load_state_dict(sd)
    env._in_rollout = False
    other = _env(*_cfgs(N + 32, 23)[:2])
    with pytest.raises(ValueError, match="num_envs"):
        other.load_state_dict(sd)
    bad = dict(sd, meta=dict(sd["meta"], version=99))
    with pytest.raises(ValueError, match="version"):
        env.load_state_dict(bad)
    # no host synchronisation in the snapshot
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        env.state_dict()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    env.load_state_dict(sd)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ whole runs
KEYS4 = {"model_state_dict", "optimizer_state_dict", "iter", "infos"}


def _runner(tmp, num_envs=64, seed=31, exact=True, presteps=0, save_interval=2):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    PPO.precision = "bf16"
    args, env_cfg, train_cfg = _cfgs(num_envs, seed)
    _short_episodes(env_cfg)                        # resets, resamples and pushes inside every rollout
    train_cfg.runner.save_interval = save_interval
    if exact:
        train_cfg.runner.exact_resume = True
    env = _env(args, env_cfg)
    if presteps:                                    # NOT the constructed state: other episodes, other counters, another seek() base
        g = torch.Generator().manual_seed(99)
        for _ in range(presteps):
            env.step((torch.randn(num_envs, 12, generator=g) * 0.4).cuda())
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    return runner


def _run_state(r):
    torch.cuda.synchronize()
    alg, net = r.alg, r.alg.net
    return dict(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone(), opt01=net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(),
                sample_step=alg._sample_step.clone(), perm_draws=torch.tensor([alg._perm_draws, int(alg._perm_draws_dev)]),
                iteration=torch.tensor(r.current_learning_iteration), obs_slot0=alg.storage._obs_all[0].clone(),
                priv_slot0=alg.storage._priv_all[0].clone()), r.env.state_dict()


def _exact_regime(runner, what):
    """The last step of the last rollout in which an env reset had at most two of them: extras["episode"] is then an exact sum (module
    docstring).  Deterministic for the seed; should another seed or size break it, choose one that does not -- do not drop the figure."""
    d = runner.alg.storage.dones.view(runner.num_steps_per_env, -1).sum(dim=1)
    steps = d.nonzero().flatten()
    assert steps.numel() == 0 or int(d[steps[-1]]) <= 2, "%s: %d envs reset in the last resetting step of the rollout" % (what, int(d[steps[-1]]))


def _compare_runs(u, r, what, env_skip=()):
    (su, eu), (sr, er) = u, r
    for k in su:
        assert torch.equal(su[k], sr[k]), "%s: `%s` differs (%s vs %s)" % (what, k, su[k].flatten()[:4].tolist(), sr[k].flatten()[:4].tolist())
    _same_state(eu, er, what + ": env", skip=env_skip)


def _uninterrupted(tmp, **kw):
    u = _runner(tmp, **kw)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    return u


def _resumed(tmp, path, iterations=1, **kw):
    r = _runner(tmp, presteps=3, **kw)
    r.load(path)
    assert r.current_learning_iteration == 3 and r.alg._perm_draws == 3 and int(r.alg._sample_step) == 3 * r.num_steps_per_env
    r.learn(num_learning_iterations=iterations, init_at_random_ep_len=True)
    r.wait_for_saves()
    return r


def test_resumed_run_is_the_run_default_plan(tmp_path):
    """Fused rollout, both HIP graphs, background writer.  U: learn(4), checkpoints every 2.  R: a fresh env that has already stepped,
    a fresh runner, load(model_2.pt) -- the sidecar says 3 iterations are done -- and learn(1)."""
    u = _uninterrupted(tmp_path / "u")
    assert u.env.rollout_fused_mode(u.alg.net) == "inline" and u._graph is not None and u._update_graph is not None
    files = sorted(os.listdir(u.log_dir))
    for it in (0, 2, 4):
        assert "model_%d.pt" % it in files and "envstate_%d.pt" % it in files, files
    assert not [f for f in files if ".tmp" in f]
    side = torch.load(os.path.join(u.log_dir, "envstate_2.pt"), map_location="cpu")
    assert side["iterations_done"] == 3 and side["num_steps_per_env"] == u.num_steps_per_env and (side["world_size"], side["rank"]) == (1, 0)
    assert torch.load(os.path.join(u.log_dir, "envstate_0.pt"), map_location="cpu")["iterations_done"] == 1
    assert torch.load(os.path.join(u.log_dir, "envstate_4.pt"), map_location="cpu")["iterations_done"] == 4
    ck = torch.load(os.path.join(u.log_dir, "model_2.pt"), map_location="cpu")
    assert set(ck) == KEYS4 and ck["iter"] == 0          # (the reference's stale count: why the sidecar carries its own)
    assert int(side["env"]["counters"][L.CNT_STEP]) == 1 + 3 * u.num_steps_per_env
    r = _resumed(tmp_path / "r", os.path.join(u.log_dir, "model_2.pt"))
    assert r.current_learning_iteration == 4 and r._graph is None        # (R's one iteration ran eagerly; U's fourth was a graph replay)
    _exact_regime(u, "default plan")
    _compare_runs(_run_state(u), _run_state(r), "default plan")
    # the final checkpoints of the two runs agree as well
    a = torch.load(os.path.join(u.log_dir, "envstate_4.pt"), map_location="cpu")
    b = torch.load(os.path.join(r.log_dir, "envstate_4.pt"), map_location="cpu")
    _same_state(a["env"], b["env"], "envstate_4.pt")
    ma, mb = (torch.load(os.path.join(x.log_dir, "model_4.pt"), map_location="cpu") for x in (u, r))
    assert all(torch.equal(ma["model_state_dict"][k], mb["model_state_dict"][k]) for k in ma["model_state_dict"])
    # two more iterations on both: still the same run (R captures its graphs now)
    u.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    r.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    u.wait_for_saves()
    _exact_regime(u, "default plan, two iterations later")
    _compare_runs(_run_state(u), _run_state(r), "default plan, two iterations later")


PLANS = {
    "eager": dict(HGYM_GRAPH="0", HGYM_GRAPH_UPDATE="0"),
    "stepwise": dict(HGYM_FUSE_ROLLOUT="0"),
    "deferred": dict(HGYM_ROLLOUT_CRITIC="deferred"),
    "default": dict(),
}


def _set_plan(monkeypatch, plan):
    for k in ("HGYM_GRAPH", "HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_ROLLOUT_CRITIC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)


# Across plans: the captured graphs replay the eager launches (test_captured_update_equals_eager_update) and the fused launch computes
# what act + step compute (test_fused_rollout_step_equals_act_then_step), both asserted bit-identical, so a checkpoint of one resumes
# under the other.  The deferred critic is NOT paired with the others: its values come from 64-row tiles over the stored rows, which
# the existing suite compares to the inline critic's within 1e-6, not bit for bit.
@pytest.mark.parametrize("plan_u,plan_r", [("eager", "eager"), ("stepwise", "stepwise"), ("deferred", "deferred"),
                                           ("default", "eager"), ("eager", "default"), ("default", "stepwise")])
def test_resumed_run_is_the_run_other_plans(tmp_path, monkeypatch, plan_u, plan_r):
    _set_plan(monkeypatch, plan_u)
    u = _uninterrupted(tmp_path / "u")
    mode = u.env.rollout_fused_mode(u.alg.net)
    want = dict(eager="inline", stepwise="inline", deferred="deferred", default="inline")[plan_u]
    assert mode == want and (u._graph is None) == (plan_u == "eager")
    _exact_regime(u, plan_u)
    state_u = _run_state(u)
    _set_plan(monkeypatch, plan_r)
    r = _resumed(tmp_path / "r", os.path.join(u.log_dir, "model_2.pt"))
    # Across plans two things belong to the path that stepped last, not to the run: the output-set flip (host book-keeping, in meta),
    # and, between the fused launch and act + step, the ALTERNATE rew / reset / time_out set, which only the fused launch writes
    # (test_fused_rollout_step_equals_act_then_step compares the primary set for the same reason).  No later step reads either.
    skip = () if plan_u == plan_r else ("meta",) if "stepwise" not in (plan_u, plan_r) else ("meta", "rew_alt", "reset_alt", "time_out_alt")
    _compare_runs(state_u, _run_state(r), "%s -> %s" % (plan_u, plan_r), env_skip=skip)


def test_off_means_off(tmp_path, monkeypatch):
    """No switch: no sidecar, load() is today's load(), and model_<it>.pt holds what the synchronous torch.save writes."""
    u = _runner(tmp_path / "u", exact=False)
    u.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    u.wait_for_saves()
    files = sorted(os.listdir(u.log_dir))
    assert not [f for f in files if f.startswith("envstate")] and {"model_0.pt", "model_2.pt", "model_3.pt"} <= set(files)
    assert getattr(u, "_snapshot", None) is not None and all("env" not in b for b in u._snapshot.sets)      # nothing pinned for it either
    # load() without a sidecar: the env keeps its state, except counters[0] (seek)
    r = _runner(None, exact=False, presteps=3)
    before = r.env.state_dict()
    r.load(os.path.join(u.log_dir, "model_3.pt"))
    after = r.env.state_dict()
    assert int(after["counters"][L.CNT_STEP]) == r.env._seek_base + 3 * r.num_steps_per_env and r.current_learning_iteration == 3
    assert torch.equal(after["counters"][1:], before["counters"][1:])
    _same_state(before, after, "load() without a sidecar", skip=("counters",))
    assert not r._keep_episode_lengths
    # the background model file against the synchronous one (as test_background_checkpoint_equals_the_synchronous_one)
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "0")
    u.save(str(tmp_path / "sync.pt"))
    a = torch.load(str(tmp_path / "sync.pt"), map_location="cpu")
    b = torch.load(os.path.join(u.log_dir, "model_3.pt"), map_location="cpu")
    assert set(a) == set(b) == KEYS4 and a["iter"] == b["iter"] == 3
    assert list(a["model_state_dict"]) == list(b["model_state_dict"])
    for k in a["model_state_dict"]:
        assert torch.equal(a["model_state_dict"][k], b["model_state_dict"][k]), k
    oa, ob = a["optimizer_state_dict"], b["optimizer_state_dict"]
    assert oa["param_groups"] == ob["param_groups"] and sorted(oa["state"]) == sorted(ob["state"])
    for i in oa["state"]:
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(oa["state"][i][f], ob["state"][i][f]), (i, f)
    assert not os.path.exists(str(tmp_path / "envstate_sync.pt"))


def test_load_optimizer_false_keeps_its_meaning_without_the_switch(tmp_path):
    """A sidecar is there, the run did not ask for exact_resume: load(path, load_optimizer=False) restores the env and the count but
    leaves Adam's state alone; with the switch the optimiser is loaded regardless."""
    u = _runner(tmp_path / "u")
    u.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    u.wait_for_saves()
    path = os.path.join(u.log_dir, "model_1.pt")
    assert os.path.exists(u.env_state_path(path))
    plain = _runner(None, exact=False)
    plain.load(path, load_optimizer=False)
    torch.cuda.synchronize()
    assert plain.current_learning_iteration == 1 and float(plain.alg.net.adam_v.abs().max()) == 0.0 and int(plain.alg.net.opt_state[L.OPT_STEP]) == 0
    _same_state(plain.env.state_dict(), u.env.state_dict(), "env restored")
    exact = _runner(None, exact=True)
    exact.load(path, load_optimizer=False)
    torch.cuda.synchronize()
    assert torch.equal(exact.alg.net.adam_v, u.alg.net.adam_v) and torch.equal(exact.alg.net.opt_state[L.OPT_LR:L.OPT_STEP + 1], u.alg.net.opt_state[L.OPT_LR:L.OPT_STEP + 1])
    ignored = _runner(None, exact=True, presteps=2)
    before = ignored.env.state_dict()
    ignored.load(path, env_state=False)                  # today's load(), sidecar or not
    _same_state(before, ignored.env.state_dict(), "env_state=False", skip=("counters",))
    small = _runner(None, num_envs=32)                  # a sidecar of another env size: refused before the parameters change
    p0 = small.alg.net.params.clone()
    with pytest.raises(ValueError, match="num_envs"):
        small.load(path)
    assert torch.equal(small.alg.net.params, p0) and small.current_learning_iteration == 0


def test_synchronous_and_background_sidecars_agree(tmp_path, monkeypatch):
    u = _runner(None)
    u.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "0")
    u.save(str(tmp_path / "model_sync.pt"), env_state=True)
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "1")
    u.save(str(tmp_path / "model_async.pt"), env_state=True)          # wait=True: on disk when the call returns
    u.save(str(tmp_path / "model_async2.pt"), env_state=True)         # (the second pinned set)
    a, b, c = (torch.load(str(tmp_path / ("envstate_%s.pt" % n)), map_location="cpu") for n in ("sync", "async", "async2"))
    for other in (b, c):
        assert {k: v for k, v in a.items() if k != "env"} == {k: v for k, v in other.items() if k != "env"}
        assert a["iterations_done"] == 2
        _same_state(a["env"], other["env"], "sidecars")
    _same_state(a["env"], {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in u.env.state_dict().items()}, "sidecar vs the live env")
    for n in ("sync", "async"):
        assert set(torch.load(str(tmp_path / ("model_%s.pt" % n)), map_location="cpu")) == KEYS4
    # the training thread only enqueues: the pinned sets are pinned, and the snapshot copies do not synchronise
    assert all(t.is_pinned() for bset in u._snapshot.sets for t in bset["env"].values())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        u.env.state_dict(out=u._snapshot.sets[0]["env"])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
