"""Records LeggedRobot.reset_idx(env_ids) for a SUBSET of envs from the unmodified reference on CPU (legged_robot.py:163-215 +
humanoid_env.py:264-269), called from the host between two steps, the way play scripts and custom tasks do.  Two cases:

  tests/golden/reset_idx_trace.npz          the XBot-L defaults;
  tests/golden/reset_idx_trace_generic.npz  a trimesh terrain map (custom origins with spawn jitter, terrain curriculum, height
                                            measurements) and the command curriculum, common_step_counter a multiple of
                                            max_episode_length when reset_idx runs, so the command curriculum is decided INSIDE the
                                            partial reset (on the listed envs' episode sums, before the commands are resampled).

Each holds
  warm-up   S0 steps (inputs, draws, outputs), as gen_fixtures.py::gen_env_reset_trace records them;
  reset     reset_idx(ids) for an unsorted, non-contiguous id list holding env 0 and env N-1; its draws scattered to env-indexed
            tables (u_dof, u_cmd[:, 3:6]; generic: r_level, u_xy); the full state right after it;
  steps     two steps with their draws and outputs; a listed env is reset AGAIN in the first one (a base-link contact).

Deterministic: a re-run reproduces each file byte for byte (seeded generators, one CPU thread, compressed with fixed names).
    python tests/golden/gen_reset_idx_fixture.py [out_dir]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402

torch.set_num_threads(1)

IDS = [9, 0, 4, 15, 11, 6]       # unsorted, non-contiguous, env 0 and env N-1 among them


def npy(t):
    return t.detach().cpu().numpy().copy()


def gen_reset_idx_trace(out_dir=HERE, N=16, S0=3, seed=17, name="reset_idx_trace.npz", generic=False):
    torch.manual_seed(seed)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    fr = 0.1 + 1.9 * torch.rand(N, 1, generator=g)
    bm = 15.0 + 10.0 * torch.rand(N, 1, generator=g) - 5.0
    if generic:
        e, cfg = H.make_ref_env(N, frictions=fr, body_mass=bm, terrain=H.TERRAIN_OPTS, command_curriculum=True)
    else:
        e, cfg = H.make_ref_env(N, frictions=fr, body_mass=bm)
    ids_log = []
    orig_resample, orig_reset_dofs = e._resample_commands, e._reset_dofs

    def resample(env_ids):
        ids_log.append(("cmd", env_ids.clone()))
        return orig_resample(env_ids)

    def reset_dofs(env_ids):
        ids_log.append(("dof", env_ids.clone()))
        return orig_reset_dofs(env_ids)

    e._resample_commands, e._reset_dofs = resample, reset_dofs

    def take(log, prefix):
        tag, t = log.pop(0)
        assert tag.startswith(prefix), (tag, prefix)
        return t

    def scatter(ids, vals, width):
        full = torch.zeros(N, width)
        if len(ids):
            full[ids] = vals.view(len(ids), width)
        return full

    if generic:
        levels0, origins0 = e.terrain_levels.clone(), e.env_origins.clone()
    H.RECORDER.enabled = True
    with H.recording_rng():
        H.finish_init(e)
    log = H.RECORDER.pop_all()
    del ids_log[:]
    out = dict(friction=npy(fr), body_mass=npy(bm), ids=np.array(IDS, dtype=np.int64))
    if generic:                    # the layout of env_trace_generic.npz (env_common.terrain_spec_from_golden reads it)
        t0 = e.terrain
        out.update(terrain_origins=npy(e.terrain_origins), terrain_types=npy(e.terrain_types), terrain_levels0=npy(levels0),
                   height_samples=t0.heightsamples.astype(np.int16), height_points=npy(e.height_points[0]),
                   terrain_env_length=np.array(t0.env_length), terrain_border=np.array(float(cfg.terrain.border_size)),
                   terrain_hscale=np.array(cfg.terrain.horizontal_scale), terrain_vscale=np.array(cfg.terrain.vertical_scale),
                   max_curriculum=np.array(cfg.commands.max_curriculum), env_origins0=npy(origins0))
        out["prime_r_level"] = npy(take(log, "randint_like"))
    out["prime_u_dof"] = npy(take(log, "rand_float"))
    if generic:
        out["prime_u_xy"] = npy(take(log, "rand_float"))
    out["prime_u_cmd"] = npy(torch.cat([take(log, "rand_float") for _ in range(3)], dim=1))
    out["prime_z_obs"] = npy(take(log, "randn_like"))
    assert not log
    ep = torch.randint(5, 2000, (N,), generator=g)
    ep[0:3] = torch.tensor([2399, 798, 2397])               # a time-out and a command resample inside the warm-up
    e.episode_length_buf = ep.clone()
    # generic: the counter reaches 2400 with the last warm-up step, so the partial reset after it examines the command curriculum
    e.common_step_counter = 2400 - S0 if generic else 40
    out["init_ep_len"] = npy(ep)
    out["init_common_step_counter"] = int(e.common_step_counter)
    frames = [H.synth_sim_state(g, N) for _ in range(S0 + 2)]
    frames[S0][2].view(N, H.NUM_BODIES, 3)[[4, 7], 0, 2] = 3.0     # env 4 (listed) and env 7 (not) terminate in the first step after
    counter = {"n": 0, "t": 0}

    def place_on_terrain(frame):
        """Root positions relative to the env's CURRENT origin: far (promotes), near (demotes), in between."""
        root = frame[0]
        r = torch.rand(N, generator=g)
        rad = torch.where(r < 0.35, 4.2 + 2.8 * torch.rand(N, generator=g),
                          torch.where(r < 0.7, 0.3 * torch.rand(N, generator=g), 1.0 + 2.5 * torch.rand(N, generator=g)))
        ang = 6.2831853 * torch.rand(N, generator=g)
        root[:, 0] = e.env_origins[:, 0] + rad * torch.cos(ang)
        root[:, 1] = e.env_origins[:, 1] + rad * torch.sin(ang)
        root[:, 2] += e.env_origins[:, 2]

    def simulate(sim):
        counter["n"] += 1
        if counter["n"] % cfg.control.decimation == 0:
            H.write_sim_state(e, frames[counter["t"]])

    e.gym.simulate = simulate

    def split_step_draws(log, ids, reset):
        u_delay = take(log, "rand(").view(N)
        z_act = take(log, "randn_like")
        kind, cb_ids = ids.pop(0)
        assert kind == "cmd"
        u_cmd = torch.zeros(N, 6)
        u_cmd[:, 0:3] = scatter(cb_ids, torch.cat([take(log, "rand_float") for _ in range(3)], dim=1), 3)
        pushed = (e.common_step_counter % cfg.domain_rand.push_interval == 0)
        u_push = torch.zeros(N, 5)
        if pushed:
            u_push[:, 0:2] = take(log, "rand_float")
            u_push[:, 2:5] = take(log, "rand_float")
        u_dof = torch.zeros(N, 12)
        u_xy, r_level = torch.zeros(N, 2), torch.zeros(N, dtype=torch.long)
        if bool(reset.any()):
            kind, r_ids = ids.pop(0)
            assert kind == "dof"
            if generic:
                r_level[r_ids] = take(log, "randint_like")
            u_dof = scatter(r_ids, take(log, "rand_float"), 12)
            if generic:
                u_xy = scatter(r_ids, take(log, "rand_float"), 2)
            kind, r_ids2 = ids.pop(0)
            assert kind == "cmd" and torch.equal(r_ids, r_ids2)
            u_cmd[:, 3:6] = scatter(r_ids, torch.cat([take(log, "rand_float") for _ in range(3)], dim=1), 3)
        z_obs = take(log, "randn_like")
        assert not log and not ids, (log, ids)
        d = dict(u_delay=u_delay, z_act=z_act, u_cmd=u_cmd, u_dof=u_dof, u_push=u_push, z_obs=z_obs)
        if generic:
            d.update(u_xy=u_xy, r_level=r_level)
        return d

    def generic_state():
        return dict(terrain_levels=e.terrain_levels, env_origins=e.env_origins, measured_heights=e.measured_heights,
                    cmd_range_x=torch.tensor([float(v) for v in e.command_ranges["lin_vel_x"]], dtype=torch.float64)) if generic else {}

    def outputs(obs, priv, rew, reset, extras):
        d = dict(obs=obs, priv=priv, rew=rew, reset=reset, time_out=e.time_out_buf, commands=e.commands, ep_len=e.episode_length_buf,
                 episode_sums=torch.stack([e.episode_sums[k] for k in e.reward_names], dim=1), torques=e.torques, actions=e.actions,
                 extras_time_outs=extras["time_outs"],
                 extras_episode=torch.stack([extras["episode"]["rew_" + k] for k in e.reward_names]),
                 root_after=e.root_states, dof_after=e.dof_state)
        d.update(generic_state())
        return d

    def run_steps(prefix, t0, n):
        rec = {}
        for t in range(t0, t0 + n):
            counter["t"] = t
            a_in = torch.randn(N, 12, generator=g) * 1.5
            if generic:
                place_on_terrain(frames[t])
            with H.recording_rng():
                res = e.step(a_in.clone())
            log, ids = H.RECORDER.pop_all(), ids_log[:]
            del ids_log[:]
            vals = dict(actions_in=a_in, root=frames[t][0], dof=frames[t][1], contact=frames[t][2], rigid=frames[t][3])
            vals.update(split_step_draws(log, ids, res[3]))
            vals.update(outputs(*res))
            for k, v in vals.items():
                rec.setdefault(k, []).append(npy(v))
        for k, v in rec.items():
            out[prefix + k] = np.stack(v)

    run_steps("warm_", 0, S0)
    ids = torch.tensor(IDS)
    if generic:
        assert e.common_step_counter % e.max_episode_length == 0
        # the listed envs tracked the commanded velocity well, the others badly: the mean over the LISTED envs widens the range
        k = "tracking_lin_vel"
        e.episode_sums[k][:] = 10.0 * torch.rand(N, generator=g) + 1.0
        e.episode_sums[k][ids] = 10.0 * torch.rand(len(IDS), generator=g) + 200.0
        out["plant_tracking_lin_vel"] = npy(e.episode_sums[k])
        # the pre-reset base positions the terrain curriculum judges: far from the origin (promote) and on it (demote)
        far = torch.arange(N) % 2 == 0
        e.root_states[:, 0] = e.env_origins[:, 0] + torch.where(far, torch.full((N,), 6.0), torch.full((N,), 0.05))
        e.root_states[:, 1] = e.env_origins[:, 1]
        out["plant_root"] = npy(e.root_states)
        range0 = [float(v) for v in e.command_ranges["lin_vel_x"]]
        levels_before = e.terrain_levels.clone()
    # ---- reset_idx(ids) from the host
    with H.recording_rng():
        e.reset_idx(ids)
    log, idl = H.RECORDER.pop_all(), ids_log[:]
    del ids_log[:]
    kind, r_ids = idl.pop(0)
    assert kind == "dof" and torch.equal(r_ids, ids)
    if generic:
        r_level = torch.zeros(N, dtype=torch.long)
        r_level[ids] = take(log, "randint_like")
        out["reset_r_level"] = npy(r_level)
    out["reset_u_dof"] = npy(scatter(ids, take(log, "rand_float"), 12))
    if generic:
        out["reset_u_xy"] = npy(scatter(ids, take(log, "rand_float"), 2))
    kind, r_ids = idl.pop(0)
    assert kind == "cmd" and torch.equal(r_ids, ids) and not idl
    u_cmd = torch.zeros(N, 6)
    u_cmd[:, 3:6] = scatter(ids, torch.cat([take(log, "rand_float") for _ in range(3)], dim=1), 3)
    out["reset_u_cmd"] = npy(u_cmd[:, 3:6])
    assert not log
    if generic:
        assert [float(v) for v in e.command_ranges["lin_vel_x"]] != range0, "the command curriculum did not fire inside reset_idx"
        d = e.terrain_levels - levels_before
        assert bool((d > 0).any()) and bool((d < 0).any()), "the terrain curriculum did not move levels both ways"
    after = dict(commands=e.commands, ep_len=e.episode_length_buf, root=e.root_states, dof=e.dof_state, reset=e.reset_buf,
                 episode_sums=torch.stack([e.episode_sums[k] for k in e.reward_names], dim=1), actions=e.actions,
                 last_actions=e.last_actions, last_last_actions=e.last_last_actions, last_dof_vel=e.last_dof_vel,
                 feet_air_time=e.feet_air_time, projected_gravity=e.projected_gravity, base_euler=e.base_euler_xyz,
                 extras_time_outs=e.extras["time_outs"],
                 extras_episode=torch.stack([e.extras["episode"]["rew_" + k] for k in e.reward_names]),
                 obs_history=torch.stack(list(e.obs_history), dim=1).abs().amax(dim=(1, 2)),         # per env: zero for the listed rows
                 critic_history=torch.stack(list(e.critic_history), dim=1).abs().amax(dim=(1, 2)))
    after.update(generic_state())
    for k, v in after.items():
        out["after_" + k] = npy(v)
    run_steps("step_", S0, 2)
    assert bool(out["step_reset"][0][4]) and bool(out["step_reset"][0][7])
    H.RECORDER.enabled = False
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print("%s N=%d ids=%s | size=%.3f MB" % (name, N, IDS, os.path.getsize(path) / 1e6))
    return path


if __name__ == "__main__":
    H.load_reference()
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    gen_reset_idx_trace(out_dir)
    gen_reset_idx_trace(out_dir, seed=19, name="reset_idx_trace_generic.npz", generic=True)
