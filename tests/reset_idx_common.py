"""Shared driver of the partial-reset tests (LeggedRobot.reset_idx(env_ids) for a subset of envs, hgym_env_reset_idx): the call on the
env parity harness of env_common.py, a snapshot of every per-env buffer, and the comparisons after the call."""
import ctypes as C

import numpy as np
import torch

import env_common as EC


def reset_idx_call(env, ids, u_dof=None, u_cmd3=None, u_xy=None, r_level=None):
    """hgym_env_reset_idx on an env_common.EnvUnderTest (HIP backend) with the given device ids and optional draw tables."""
    from hgym import _lib as L
    b, N = env.buf, env.buf.N
    u_cmd = None
    if u_cmd3 is not None:
        u_cmd = torch.zeros(N, 6)
        u_cmd[:, 3:6] = u_cmd3
    noise = env._noise(u_dof=u_dof, u_cmd=u_cmd, u_xy=u_xy, r_level=r_level)
    ids_d = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).to(env.dev).contiguous()
    c0 = b.counters.cpu().clone()
    L.check(L.lib.hgym_env_reset_idx(C.byref(env.cfg), C.byref(env.sim), C.byref(env.st), C.byref(env.out), C.byref(noise),
                                     L.i64ptr(ids_d), int(ids_d.numel()), L.u8ptr(b.reset_idx_mask), L.i64ptr(b.reset_idx_rejected),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_env_reset_idx")
    torch.cuda.synchronize()
    c1 = b.counters.cpu()
    # the step counter and the ring step stay put, the reset count is cleared, the host-reset call number advances by one
    assert int(c1[0]) == int(c0[0]) and int(c1[2]) == int(c0[2]), "reset_idx moved a step counter: %s -> %s" % (c0.tolist(), c1.tolist())
    assert int(c1[1]) == 0 and int(c1[3]) == int(c0[3]) + 1, "reset count / call number: %s -> %s" % (c0.tolist(), c1.tolist())


def reset_mask(env_ids, num_envs):
    """The envs a partial reset_idx resets, as a bool (num_envs,) CPU tensor: negative ids wrapped, repeats once, ids outside
    [-num_envs, num_envs) skipped -- what hgym_env_reset_idx's mask launch builds on the device."""
    t = torch.as_tensor(np.asarray(env_ids.cpu() if torch.is_tensor(env_ids) else env_ids)).reshape(-1).to(torch.int64)
    t = t[(t >= -num_envs) & (t < num_envs)]
    m = torch.zeros(num_envs, dtype=torch.bool)
    m[torch.where(t < 0, t + num_envs, t)] = True
    return m


def snapshot(b):
    """Every per-env buffer of an EnvBuffers, env-major (row e = env e), cloned."""
    d = dict(state=b._state.t(), episode_length=b.episode_length, reset=b.reset, time_out=b.time_out, rew=b.rew,
             obs_ring=b.obs_ring, priv_ring=b.priv_ring, root=b.root_view(), dof_pos=b.dof_pos_view(), dof_vel=b.dof_vel_view(),
             contact=b.contact_view(), rigid=b.rigid_view(), obs=b.obs, priv_obs=b.priv_obs)
    if b.terrain_levels is not None:
        d["terrain_levels"] = b.terrain_levels
    if b.custom_sums is not None:
        d["custom_sums"] = b.custom_sums.t()
    if b.measured_heights is not None:
        d["measured_heights"] = b.measured_heights
    return {k: v.detach().clone() for k, v in d.items()}


def check_untouched(b, before, m, tag):
    """Rows of envs outside the mask m are bit-identical to the snapshot; no observation row was written at all."""
    now = snapshot(b)
    keep = ~m.to(now["state"].device)
    for k, v in now.items():
        if k in ("obs", "priv_obs"):
            assert torch.equal(v, before[k]), "%s: %s written by reset_idx" % (tag, k)
        else:
            assert torch.equal(v[keep], before[k][keep]), "%s: %s changed for an env outside the set" % (tag, k)


def compare_reset(env, o, m, tag):
    """The state right after a partial reset against the oracle's _reset_masked."""
    b = env.buf
    mm = m.to(b.obs_ring.device)
    EC.exact(b.reset, o.reset, tag + " reset")
    EC.exact(b.episode_length, o.ep_len, tag + " episode_length")
    EC.exact(b.extras_time_outs, o.extras_time_outs, tag + " extras time_outs")
    for name in ("commands", "actions", "last_actions", "last_last_actions", "last_dof_vel", "feet_air_time", "episode_sums",
                 "projected_gravity"):
        EC.close(b.view(name), getattr(o, name), tag + " " + name)
    EC.close(b.view("base_euler")[mm], o.base_euler[m], tag + " base_euler of the reset envs")
    EC.close(b.root_view(), o.sim.root, tag + " root")
    EC.close(b.dof_pos_view(), o.sim.dof_pos, tag + " dof_pos")
    EC.close(b.dof_vel_view(), o.sim.dof_vel, tag + " dof_vel")
    EC.close(b.extras_episode, o.extras_episode, tag + " extras episode means", rtol=1e-5, atol=1e-7)
    assert float(b.obs_ring[mm].abs().max()) == 0.0 and float(b.priv_ring[mm].abs().max()) == 0.0, tag + " history rows not zeroed"
    if o.terrain is not None:
        EC.exact(b.terrain_levels, o.terrain.levels, tag + " terrain_levels")
        EC.exact(b.view("env_origins").contiguous().view(torch.int32), o.env_origins.contiguous().view(torch.int32), tag + " env_origins")
    if o.command_curriculum:
        assert [float(v) for v in b.command_range_x.cpu()] == o.cmd_range_x, tag + " command range"


def subset(g, N, k):
    """k distinct envs in a shuffled order, with env 0 and env N - 1 among them when k >= 2; one id given negative (wrapped) and one
    repeated when k >= 3."""
    perm = torch.randperm(N, generator=g)[:k].tolist()
    if k >= 2:
        for must in (0, N - 1):
            if must not in perm:
                perm[perm.index(next(p for p in perm if p not in (0, N - 1)))] = must
    ids = list(perm)
    if k >= 3:
        ids[1] = ids[1] - N
        ids.insert(len(ids) // 2, perm[2])
    return ids
