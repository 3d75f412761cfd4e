"""-m gpu: LeggedRobot.reset_idx(env_ids) for a subset of envs (hgym_env_reset_idx; legged_robot.py:163-215 + humanoid_env.py:264-269).

  * seeded random subsets against the oracle's _reset_masked (parity mode: the draws come in as env-indexed tables), then a step;
  * the same with the generic options (trimesh terrain, terrain and command curricula) and with user-defined reward terms;
  * the recorded reference reset_idx(ids) (tests/golden/reset_idx_trace*.npz, gen_reset_idx_fixture.py), defaults and generic options;
  * the drop-in surface: id forms, range errors, guards, no host synchronisation, the draw stream, the runner around it."""
import os

import numpy as np
import pytest
import torch

import env_common as EC
import reset_idx_common as RC
from oracle import xbot_constants as K
from hgym import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return EC.HipBackend()


def _mask(ids, N):
    return RC.reset_mask(ids, N)


def _step_both(env, o, g, generic=False, tag="step"):
    N = env.buf.N
    frame = EC.synth_frames(g, N)
    a = torch.randn(N, 12, generator=g)
    nz = [torch.rand(N, generator=g), torch.randn(N, 12, generator=g), torch.rand(N, 6, generator=g), torch.rand(N, 12, generator=g),
          torch.rand(N, 5, generator=g), torch.randn(N, 47, generator=g)]
    extra = [torch.rand(N, 2, generator=g), torch.randint(0, o.terrain.max_level, (N,), generator=g)] if generic else []
    o.pre_physics(a.clone(), nz[0], nz[1])
    o.pd_torques()
    o.sim.load(*frame)
    o.post_physics(*nz[2:], *extra)
    env.step(a, frame, *nz, *extra)
    EC.compare_state(env, o, tag)


@pytest.mark.parametrize("N", [300, 4096, 8192])
def test_random_subsets_against_oracle_gpu(hip, N):
    """Subsets of 1, a few, about half and N - 1 envs (unsorted, a negative id, a repeat), each followed by one step; every env outside
    the subset keeps every buffer bit for bit."""
    counts, env, o = EC.run_random_trace(hip, N, steps=2, seed=40 + N, check_every=2)
    g = torch.Generator().manual_seed(N)
    for k in (1, 5, N // 2, N - 1):
        ids = RC.subset(g, N, k)
        m = _mask(ids, N)
        assert int(m.sum()) == k
        u_dof, u_cmd3 = torch.rand(N, 12, generator=g), torch.rand(N, 3, generator=g)
        before = RC.snapshot(env.buf)
        o._reset_masked(m, u_dof, u_cmd3)
        RC.reset_idx_call(env, ids, u_dof, u_cmd3)
        tag = "N=%d, %d envs" % (N, k)
        RC.check_untouched(env.buf, before, m, tag)
        RC.compare_reset(env, o, m, tag)
        assert int(env.buf.reset_idx_rejected) == 0 and int(env.buf.counters[L.CNT_RESETS]) == 0
        _step_both(env, o, g, tag=tag + ": the step after")


def test_generic_options_subset_gpu(hip):
    """Terrain curriculum + custom origins + height measurements, and the command curriculum firing inside the partial reset
    (common_step_counter a multiple of max_episode_length, judged on the listed envs only)."""
    N = 44
    counts, env, o = EC.run_random_trace(hip, N, steps=3, seed=321, generic=True, track_sum=5.0)
    assert o.common_step_counter % K.MAX_EPISODE_LENGTH == 0
    g = torch.Generator().manual_seed(3)
    ids = RC.subset(g, N, 9)
    m = _mask(ids, N)
    # the listed envs tracked well, the others badly: the mean over the LISTED envs moves the range
    k = K.REWARD_NAMES.index("tracking_lin_vel")
    sums = o.episode_sums.clone()
    sums[:, k] = torch.where(m, torch.full((N,), 40.0), torch.full((N,), 1.0))
    o.episode_sums = sums.clone()
    env.buf.view("episode_sums").copy_(sums)
    # positions far from / near the tile origin, so that levels go both ways
    far = torch.arange(N) % 2 == 0
    root = env.buf.root_view().cpu().clone()
    root[:, 0] = o.env_origins[:, 0] + torch.where(far, torch.full((N,), 6.0), torch.full((N,), 0.1))
    root[:, 1] = o.env_origins[:, 1]
    env.buf.root_view().copy_(root)
    o.sim.root[:] = root
    range0 = list(o.cmd_range_x)
    u_dof, u_cmd3 = torch.rand(N, 12, generator=g), torch.rand(N, 3, generator=g)
    u_xy, r_level = torch.rand(N, 2, generator=g), torch.randint(0, o.terrain.max_level, (N,), generator=g)
    levels0 = o.terrain.levels.clone()
    before = RC.snapshot(env.buf)
    o._reset_masked(m, u_dof, u_cmd3, u_xy, r_level)
    RC.reset_idx_call(env, ids, u_dof, u_cmd3, u_xy, r_level)
    assert o.cmd_range_x != range0, "the command curriculum did not fire inside the partial reset"
    assert bool((o.terrain.levels != levels0).any())
    RC.check_untouched(env.buf, before, m, "generic")
    RC.compare_reset(env, o, m, "generic")
    _step_both(env, o, g, generic=True, tag="generic: the step after")


def test_custom_reward_terms_subset_gpu(hip):
    """User-defined `_reward_<name>` terms: their episode sums are accumulated and zeroed for the listed envs only, and
    extras["episode"] of those terms is their mean over the listed envs."""
    import test_custom_rewards as TC
    from oracle.xbot_env_oracle import XBotEnvOracle
    N = 300
    g = torch.Generator().manual_seed(11)
    fr, bm = 0.1 + 1.9 * torch.rand(N, 1, generator=g), 10.0 + 10.0 * torch.rand(N, 1, generator=g)
    o = XBotEnvOracle(N, frictions=fr, body_mass=bm, extra_rewards={n: (TC.TERMS[n][1], TC.TERMS[n][0]) for n in TC.NAMES})
    env = EC.EnvUnderTest(hip, N, fr, bm)
    b, cfg = env.buf, env.cfg
    names = list(K.REWARD_NAMES)
    b.set_custom_rewards([len(names) + 1 if n == "termination" else sum(1 for x in names if x < n) for n in TC.NAMES])
    cfg.reward_scales[names.index("torques")] = 0.0
    env.sim, env.st, env.out = b.sim_struct(), b.state_struct(), b.out_struct()
    sp = TC.SplitStepBackend(hip)
    u_dof, u_cmd3, z_obs = torch.rand(N, 12, generator=g), torch.rand(N, 3, generator=g), torch.randn(N, 47, generator=g)
    o.prime(u_dof, u_cmd3, z_obs)
    env.prime(u_dof, u_cmd3, z_obs)
    hip.sync()
    for t in range(3):
        a_in = torch.randn(N, 12, generator=g) * 1.5
        frame = EC.synth_frames(g, N)
        u_delay, z_act = torch.rand(N, generator=g), torch.randn(N, 12, generator=g)
        u_cmd, u_dof = torch.rand(N, 6, generator=g), torch.rand(N, 12, generator=g)
        u_push, z_obs = torch.rand(N, 5, generator=g), torch.randn(N, 47, generator=g)
        o.pre_physics(a_in.clone(), u_delay, z_act)
        o.pd_torques()
        o.sim.load(*frame)
        o.post_physics(u_cmd, u_dof, u_push, z_obs)
        a = a_in.cuda().contiguous()
        hip.pre_physics(cfg, env.st, a, env._noise(u_delay=u_delay, z_act=z_act))
        hip.pd_torques(cfg, env.sim, env.st)
        hip.sync()
        b.load_sim(*frame)
        nz = env._noise(u_cmd=u_cmd, u_dof=u_dof, u_push=u_push, z_obs=z_obs)
        sp.begin(cfg, env.sim, env.st, env.out, nz)
        hip.sync()
        for j, n in enumerate(TC.NAMES):
            b.custom_rew[j].copy_(TC.TERMS[n][2](b) * (TC.TERMS[n][0] * K.DT))
        sp.end(cfg, env.sim, env.st, env.out, nz)
        hip.sync()
    EC.compare_state(env, o, "custom terms, before the reset")
    ids = RC.subset(g, N, 37)
    m = _mask(ids, N)
    u_dof, u_cmd3 = torch.rand(N, 12, generator=g), torch.rand(N, 3, generator=g)
    before = RC.snapshot(b)
    o._reset_masked(m, u_dof, u_cmd3)
    RC.reset_idx_call(env, ids, u_dof, u_cmd3)
    RC.check_untouched(b, before, m, "custom terms")
    RC.compare_reset(env, o, m, "custom terms")
    for j, n in enumerate(TC.NAMES):
        EC.close(b.custom_sums[j], o.extra_sums[n], "episode sum of %s after the partial reset" % n)
        EC.close(b.extras_custom[j], o.extras_extra[n], "extras of %s after the partial reset" % n, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ the recorded reference
@pytest.mark.parametrize("name", ["reset_idx_trace.npz", "reset_idx_trace_generic.npz"])
def test_reset_idx_golden_gpu(hip, golden_dir, name):
    """The reference's own reset_idx(ids) replayed from the trace gen_reset_idx_fixture.py recorded: warm-up steps, the partial reset
    with the reference's draws, the state right after it, then two steps (one of them resets a listed env again)."""
    import reset_idx_golden as RG
    RG.run_reset_idx_golden(hip, os.path.join(golden_dir, name))


# ------------------------------------------------------------------------------------------------ drop-in surface
def _make_env(num_envs=64, seed=9):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    torch.manual_seed(seed)
    np.random.seed(seed)
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    env, _ = task_registry.make_env(name=args.task, args=args)
    env.reset()
    g = torch.Generator().manual_seed(seed)
    for _ in range(3):
        env.step((torch.randn(num_envs, 12, generator=g) * 0.5).to(env.device))
    torch.cuda.synchronize()
    return env


def _env_state(env):
    b = env._buf
    return dict(state=b._state.clone(), ep=b.episode_length.clone(), counters=b.counters.clone(), obs_ring=b.obs_ring.clone(),
                priv_ring=b.priv_ring.clone(), root=b.root.clone(), dof_pos=b.dof_pos.clone(), dof_vel=b.dof_vel.clone(),
                reset=b.reset.clone(), extras_episode=b.extras_episode.clone())


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_id_forms_and_errors_gpu():
    ids = [5, 0, 63, 17, -3, 17]
    forms = [torch.tensor(ids, device="cuda"), torch.tensor(ids, dtype=torch.int32), list(ids), np.array(ids)]
    states = []
    for f in forms:
        env = _make_env()
        env.reset_idx(f)
        torch.cuda.synchronize()
        states.append(_env_state(env))
        m = _mask(ids, 64).cuda()
        assert bool(env.reset_buf[m].all()) and int(env.episode_length_buf[m].abs().sum()) == 0
        assert int(env.reset_idx_rejected) == 0
    for s in states[1:]:
        # (the episode means are sums of floats gathered with atomics: their order, hence the last bit, may differ)
        s = {k: v for k, v in s.items() if k != "extras_episode"}
        assert _same(s, {k: v for k, v in states[0].items() if k != "extras_episode"})
    # host ids out of range: IndexError before anything is launched
    env = _make_env()
    s0 = _env_state(env)
    for bad in ([1, 64], np.array([-65, 2]), torch.tensor([70])):
        with pytest.raises(IndexError):
            env.reset_idx(bad)
    with pytest.raises(IndexError):
        env.reset_idx([0.5, 1.0])
    torch.cuda.synchronize()
    assert _same(_env_state(env), s0)
    # device ids out of range: skipped on the device and counted
    env.reset_idx(torch.tensor([2, 100, -200, -1], device="cuda"))
    torch.cuda.synchronize()
    assert int(env.reset_idx_rejected) == 2
    assert bool(env.reset_buf[2]) and bool(env.reset_buf[63]) and int(env.episode_length_buf[2]) == 0
    # every id rejected: nothing reset, the extras stay as they were (no 0/0)
    ex = env._buf.extras_episode.clone()
    env.reset_idx(torch.tensor([64, -65], device="cuda"))
    torch.cuda.synchronize()
    assert int(env.reset_idx_rejected) == 2 and torch.equal(env._buf.extras_episode, ex)


def test_guards_and_no_host_sync_gpu():
    env = _make_env()
    N = env.num_envs
    dev = env.device
    sink = dict(values=torch.zeros(N, device=dev), rewards=torch.zeros(N, device=dev), dones=torch.zeros(N, dtype=torch.bool, device=dev),
                step=torch.zeros(1, dtype=torch.int64, device=dev), gamma=0.99)
    env.bind_transition(sink, defer_finalize=True)
    env.step(torch.zeros(N, 12, device=dev))
    with pytest.raises(RuntimeError):
        env.reset_idx([1, 2])
    env.run_finalize(env.take_pending_finalize())
    env.bind_transition(None)
    env._in_rollout = True                # what rollout_begin leaves until rollout_end
    with pytest.raises(RuntimeError):
        env.reset_idx([1, 2])
    env._in_rollout = False
    ids = torch.tensor([4, 9, 33], device=dev)
    ids32 = ids.to(torch.int32)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        env.reset_idx(ids)
        env.reset_idx(ids32)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert int(env.episode_length_buf[ids].abs().sum()) == 0


def test_draw_stream_gpu():
    env = _make_env()
    dev = env.device
    c0 = env._buf.counters.clone()
    env.reset_idx([3, 8])
    d1 = env.dof_pos[3].clone()
    env.reset_idx([3, 8])
    d2 = env.dof_pos[3].clone()
    torch.cuda.synchronize()
    c = env._buf.counters.cpu()
    assert int(c[3]) == int(c0[3]) + 2 and int(c[0]) == int(c0[0]) and int(c[2]) == int(c0[2])
    assert not torch.equal(d1, d2), "two host resets drew the same joint offsets"
    # a host reset, then a step that resets the same env through the step kernel's mask (a time-out)
    env.reset_idx([5])
    d_host = env.dof_pos[5].clone()
    c_host = env.commands[5].clone()
    ep = env.episode_length_buf.clone()
    ep[5] = 2400
    env.episode_length_buf = ep
    _, _, _, dones, _ = env.step(torch.zeros(env.num_envs, 12, device=dev))
    torch.cuda.synchronize()
    assert bool(dones[5])
    assert not torch.equal(d_host, env.dof_pos[5]) and not torch.equal(c_host, env.commands[5])
    # the same call sequence on a fresh env with the same seed reproduces the state bit for bit
    a, b = _make_env(seed=4), _make_env(seed=4)
    for e in (a, b):
        e.reset_idx([1, 7, 7, 40])
        e.reset_idx(torch.tensor([7, 2], device=dev))
        e.step(torch.full((e.num_envs, 12), 0.1, device=dev))
        e.reset_idx(np.array([2]))
    torch.cuda.synchronize()
    sa, sb = _env_state(a), _env_state(b)
    sa.pop("extras_episode")
    sb.pop("extras_episode")
    assert _same(sa, sb)


def test_runner_around_reset_idx_gpu(tmp_path):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", "256", "--max_iterations", "2"])
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=str(tmp_path))
    assert env.rollout_fused_mode(runner.alg.net) is not None        # this configuration collects with the fused rollout launch
    calls = []
    orig = env.rollout_step

    def spy(i):                    # a partial reset between the launches of a fused rollout is refused before any launch
        if i == 1 and not calls:
            with pytest.raises(RuntimeError):
                env.reset_idx([0, 1])
            calls.append(i)
        return orig(i)

    env.rollout_step = spy
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    env.rollout_step = orig
    torch.cuda.synchronize()
    assert calls == [1], "the fused rollout never called rollout_step"
    ids = torch.tensor([0, 31, 100, 255, 77], device=env.device)
    keep = torch.ones(256, dtype=torch.bool, device=env.device)
    keep[ids] = False
    dof_other, ep_other = env.dof_pos[keep].clone(), env.episode_length_buf[keep].clone()
    env.reset_idx(ids)
    torch.cuda.synchronize()
    assert int(env.episode_length_buf[ids].abs().sum()) == 0
    off = env.dof_pos[ids] - env.default_dof_pos
    assert float(off.abs().max()) <= 0.1 + 1e-6 and float(env.dof_vel[ids].abs().max()) == 0.0
    assert torch.equal(env.dof_pos[keep], dof_other) and torch.equal(env.episode_length_buf[keep], ep_other)
    runner.learn(num_learning_iterations=2)
    torch.cuda.synchronize()
    assert torch.isfinite(runner.alg.net.params).all()
