"""GPU: the planted edge table of env_edges_common.py through the device kernels (hgym_pre_physics, hgym_pd_torques,
hgym_post_physics), against the fp32 oracle and the float64 restatement of the step; and the state-side subset of the edges through
the fused step that makes its own sim frame from Philox (hgym_env_step_synth), against oracle/synth_env_oracle.py.  Every test runs
its steps once: nothing here repeats a step that failed."""
import ctypes as C

import numpy as np
import pytest
import torch

import env_common as EC
import env_edges_common as EE
import synth_common as SC
from oracle import synth_env_oracle as S
from oracle import xbot_constants as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return EC.HipBackend()


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("pass_name,nfill", [("ones", 55), ("default", 55), ("signed", 55), ("ones", 61)])
def test_planted_edges_gpu(hip, pass_name, nfill, layout):
    """N = 154 (99 cases among 55 ordinary envs): ten workgroups of 16 envs, the last one ragged; N = 160: whole workgroups."""
    EE.run_table(hip, pass_name, sim_layout=layout, nfill=nfill)
    EE.report_errors(hip.name, pass_name)


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_clipped_frames_travel_through_the_ring_gpu(hip, layout):
    """The planted step and 15 more on the device: the prefetched older-frames copy (hist_load / hist_store) clips what it copies."""
    EE.run_table(hip, "default", sim_layout=layout, more_steps=15)


def test_state_side_edges_fused_step_gpu():
    """hgym_env_step_synth with the state-side subset of the edges planted (env_edges_common.run_fused_state_edges), N = 1000 (not a
    multiple of the workgroup's 16 envs), 18 steps with a push, time-outs and command resamples inside the window."""
    from hgym import EnvBuffers, default_env_config, _lib as L
    from oracle.xbot_env_oracle import XBotEnvOracle
    N, steps, seed = 1000, 18, 0x5EED0EDE
    g = torch.Generator().manual_seed(N + 1)
    cfg = default_env_config(N, seed=seed)
    buf = EnvBuffers(cfg, "cuda")
    buf.f["friction"].copy_((0.1 + 1.9 * torch.rand(N, generator=g)).view(1, N))
    buf.f["body_mass"].copy_((10.0 + 10.0 * torch.rand(N, generator=g)).view(1, N))
    sim, st, out, nz = buf.sim_struct(), buf.state_struct(), buf.out_struct(), buf.noise_struct()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.hgym_env_prime(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(out), C.byref(nz), s), "prime")
    torch.cuda.synchronize()
    o0 = XBotEnvOracle(N, frictions=buf.view("friction").cpu().clone(), body_mass=buf.view("body_mass").cpu().clone())
    S.synth_prime(o0, seed)
    SC.compare(buf, o0, "prime", [0])
    keep = []

    def step(a):
        keep[:] = [a.cuda()]
        L.check(L.lib.hgym_env_step_synth(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(out), L.fptr(keep[0]), s), "step")
    counts, reached, flips = EE.run_fused_state_edges(buf, step, torch.cuda.synchronize, g, seed, steps)
    SC.report("fused step (hgym_env_step_synth) with planted state-side edges vs oracle, N=%d, %d steps: %s; sim-side edges the Philox "
              "frames reached (information): %s" % (N, steps, counts, reached), flips)
    assert counts["push"] == 1 and counts["timeout"] >= 3


@pytest.mark.parametrize("ahead", [True, False])
def test_state_side_edges_rollout_step_gpu(monkeypatch, ahead):
    """hgym_rollout_step (one launch per vec-step: the four-role chain + env_step_reward_sum on real wavefronts, the older frames through
    hist_load / hist_store, rows written one launch ahead) with the state-side edges planted, 4096 envs, 20 steps, driven and compared
    the way test_synth_path.py::test_rollout_step_env_part_vs_oracle_gpu does: the policy's sampled actions are the oracle's inputs; next
    observations (the planted ring frames come out clipped), dones, bootstrapped rewards and the final env state against the oracle on
    the same Philox stream; low_speed flip budget unchanged (2)."""
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    monkeypatch.setenv("HGYM_GRAPH", "0")
    torch.manual_seed(99)
    np.random.seed(99)
    N, T = 4096, 20
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(N), "--seed", "17"])
    task_registry.train_cfgs[args.task].seed = 17
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    alg, buf = runner.alg, env._buf
    assert env.rollout_fused_supported(alg.net)
    seed = int(env._ncfg.seed)
    g = torch.Generator().manual_seed(3)
    EE.plant_state_edges(buf, g, csc=K.PUSH_INTERVAL - 10)
    torch.cuda.synchronize()
    o = SC.oracle_from_buffers(buf)
    st = alg.storage
    obs_all, priv_all = st._obs_all, st._priv_all
    obs_all[0].copy_(env.get_observations())
    priv_all[0].copy_(env.get_privileged_observations())
    alg.env_stores_transitions = True
    with torch.inference_mode():
        alg.fused_rollout_step(env, T, rows_ahead=ahead)
    torch.cuda.synchronize()
    flips, counts = 0, dict(reset=0, timeout=0, push=0)
    assert float(obs_all[1][80:84].abs().max()) == K.CLIP_OBS and float(priv_all[1][80:84].abs().max()) == K.CLIP_OBS
    for i in range(T):
        a = st.actions[i].cpu()
        obs_o, priv_o, rew_o, reset_o, info = S.synth_step(o, seed, a)
        rew_dev = st.rewards[i].view(-1).cpu()
        boot = alg.gamma * (st.values[i].view(-1).cpu() * o.extras_time_outs.float())        # ppo.py:107-108
        want = o.rew + boot
        d = (rew_dev - want).abs()
        bad = (d > (EC.ATOL + EC.RTOL * want.abs())).nonzero().flatten().tolist()
        for e in bad:                               # low_speed threshold flips (tests/synth_common.py): counted, re-synchronised
            assert float(d[e]) <= SC.LOW_SPEED_QUANTUM, (i, e, float(d[e]))
            o.rew[e] = rew_dev[e] - boot[e]
            o.episode_sums[e, K.REWARD_NAMES.index("low_speed")] += (rew_dev[e] - want[e])
        flips += len(bad)
        EC.exact(st.dones[i].view(-1), reset_o, "dones %d" % i)
        EC.close(obs_all[i + 1], obs_o, "next obs %d" % i)
        EC.close(priv_all[i + 1], priv_o, "next privileged obs %d" % i)
        counts["reset"] += int(reset_o.sum())
        counts["timeout"] += int(o.time_out.sum())
        counts["push"] += int(info["pushed"])
    assert flips <= 2, flips
    o.rew = buf.rew.cpu().clone() if flips else o.rew
    EC.compare_state(SC.Holder(buf), o, "after the rollout", check_obs=False)
    SC.report("fused rollout step (hgym_rollout_step, rows ahead: %s) with planted state-side edges vs oracle, N=%d, %d steps: %s"
              % (ahead, N, T, counts), flips)
    assert counts["push"] == 1 and counts["timeout"] >= 3


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("pass_name", list(EE.GENERIC_PASSES))
def test_generic_options_edges_gpu(hip, pass_name, layout):
    """The generic-option cases (height-map borders and corners, the yaw-quaternion norm floor, level promotion / demotion, the command
    curriculum either side of its bar and at its cap) through the device's generic chain; run_generic asserts levels, origins' bits,
    sampled heights and the command range exactly."""
    census = EE.run_generic(hip, pass_name, layout)
    assert all(n > 0 for sides in census.values() for n in sides.values()), census
