"""Replay of tests/golden/reset_idx_trace.npz and reset_idx_trace_generic.npz (gen_reset_idx_fixture.py: the reference's own
reset_idx(ids) for a subset of envs, between warm-up steps and two following steps) through the oracle (CPU) or through the HIP library
(GPU).  The generic trace (trimesh map, terrain + command curricula) also pins terrain levels, env origins and sampled heights bit for
bit and the command range exactly, with the command curriculum decided inside the partial reset."""
import numpy as np
import torch

import env_common as EC
from oracle import xbot_constants as K
from oracle.xbot_env_oracle import XBotEnvOracle
from hgym import _lib as L

Tn = lambda a: torch.from_numpy(np.asarray(a))
AFTER_FIELDS = ("commands", "actions", "last_actions", "last_last_actions", "last_dof_vel", "feet_air_time", "episode_sums",
                "projected_gravity")
TRACKING = K.REWARD_NAMES.index("tracking_lin_vel")


def _check_generic(levels, origins, heights, cmd_range, g, tag, heights_too=True):
    EC.exact(levels, g("terrain_levels"), tag + " terrain_levels")
    EC.exact(origins.contiguous().view(torch.int32), Tn(np.ascontiguousarray(g("env_origins"))).view(torch.int32), tag + " env_origins (bits)")
    if heights_too:
        EC.exact(heights.contiguous().view(torch.int32), Tn(np.ascontiguousarray(g("measured_heights"))).view(torch.int32),
                 tag + " measured_heights (bits)")
    assert [float(v) for v in cmd_range] == [float(v) for v in g("cmd_range_x")], tag + " command range"


def _check_step(b_or_o, g, tag, hip, generic):
    """One step's outputs as run_reset_golden checks them (hip: an EnvBuffers; else the oracle and its step results)."""
    if hip:
        b = b_or_o
        EC.exact(b.reset, g("reset"), tag + " reset")
        EC.exact(b.time_out, g("time_out"), tag + " time_out")
        EC.exact(b.episode_length, g("ep_len"), tag + " ep_len")
        EC.exact(b.extras_time_outs, g("extras_time_outs"), tag + " extras time_outs")
        EC.close(b.rew, g("rew"), tag + " rew")
        EC.close(b.view("torques"), g("torques"), tag + " torques", atol=2e-5)
        EC.close(b.view("actions"), g("actions"), tag + " actions")
        EC.close(b.view("commands"), g("commands"), tag + " commands")
        EC.close(b.view("episode_sums"), g("episode_sums"), tag + " episode_sums")
        EC.close(b.root, g("root_after"), tag + " root")
        EC.close(b.dof_state, g("dof_after"), tag + " dof")
        EC.close(b.extras_episode, g("extras_episode"), tag + " extras episode", rtol=1e-5, atol=1e-7)
        EC.close(b.obs, g("obs"), tag + " obs")
        EC.close(b.priv_obs, g("priv"), tag + " priv")
        if generic:
            _check_generic(b.terrain_levels, b.view("env_origins"), b.measured_heights, b.command_range_x.cpu(), g, tag)
    else:
        o, (tq, obs, priv, rew, reset) = b_or_o
        EC.exact(reset, g("reset"), tag + " reset")
        EC.exact(o.time_out, g("time_out"), tag + " time_out")
        EC.exact(o.ep_len, g("ep_len"), tag + " ep_len")
        EC.exact(o.extras_time_outs, g("extras_time_outs"), tag + " extras time_outs")
        EC.close(rew, g("rew"), tag + " rew")
        EC.close(tq, g("torques"), tag + " torques", atol=2e-5)
        EC.close(o.commands, g("commands"), tag + " commands")
        EC.close(o.episode_sums, g("episode_sums"), tag + " episode_sums")
        EC.close(o.sim.root, g("root_after"), tag + " root")
        EC.close(torch.stack((o.sim.dof_pos, o.sim.dof_vel), -1).view(-1, 2), g("dof_after"), tag + " dof")
        EC.close(o.extras_episode, g("extras_episode"), tag + " extras episode", rtol=1e-5, atol=1e-7)
        EC.close(torch.clip(obs, -K.CLIP_OBS, K.CLIP_OBS), g("obs"), tag + " obs")
        EC.close(torch.clip(priv, -K.CLIP_OBS, K.CLIP_OBS), g("priv"), tag + " priv")
        if generic:
            _check_generic(o.terrain.levels, o.env_origins, o.measured_heights, o.cmd_range_x, g, tag)


def run_reset_idx_golden(backend, path):
    """backend: env_common.HipBackend() -> the HIP library (hgym_env_reset_idx); None -> the oracle (_reset_masked)."""
    G = np.load(path)
    N = G["friction"].shape[0]
    generic = "terrain_origins" in G.files
    ids = Tn(G["ids"])
    m = torch.zeros(N, dtype=torch.bool)
    m[ids] = True
    hip = backend is not None
    prime_extra = (Tn(G["prime_u_xy"]), Tn(G["prime_r_level"])) if generic else ()
    spec = EC.terrain_spec_from_golden(G) if generic else None
    max_curr = float(G["max_curriculum"]) if generic else None
    if hip:
        import reset_idx_common as RC
        env = EC.EnvUnderTest(backend, N, Tn(G["friction"]), Tn(G["body_mass"]), sim_layout="aos", terrain=spec, command_curriculum=max_curr)
        env.prime(Tn(G["prime_u_dof"]), Tn(G["prime_u_cmd"]), Tn(G["prime_z_obs"]), *prime_extra)
        backend.sync()
        env.buf.episode_length.copy_(Tn(G["init_ep_len"]))
        env.buf.counters[L.CNT_STEP] = int(G["init_common_step_counter"])
    else:
        o = XBotEnvOracle(N, frictions=Tn(G["friction"]), body_mass=Tn(G["body_mass"]), terrain=spec, command_curriculum=generic,
                          max_curriculum=max_curr if generic else 1.0)
        o.prime(Tn(G["prime_u_dof"]), Tn(G["prime_u_cmd"]), Tn(G["prime_z_obs"]), *prime_extra)
        o.ep_len = Tn(G["init_ep_len"]).clone()
        o.common_step_counter = int(G["init_common_step_counter"])

    def step(g, tag):
        frame = (Tn(g("root")), Tn(g("dof")), Tn(g("contact")), Tn(g("rigid")))
        nz = [Tn(g(k)) for k in ("u_delay", "z_act", "u_cmd", "u_dof", "u_push", "z_obs")]
        extra = [Tn(g("u_xy")), Tn(g("r_level"))] if generic else []
        if hip:
            env.step(Tn(g("actions_in")), frame, *nz, *extra)
            _check_step(env.buf, g, tag, True, generic)
        else:
            o.pre_physics(Tn(g("actions_in")).clone(), nz[0], nz[1])
            tq = o.pd_torques()
            o.sim.load(*frame)
            obs, priv, rew, reset, _ = o.post_physics(*nz[2:], *extra)
            _check_step((o, (tq, obs, priv, rew, reset)), g, tag, False, generic)

    for t in range(G["warm_rew"].shape[0]):
        step(lambda k, t=t: G["warm_" + k][t], "warm-up step %d" % t)
    u_dof, u_cmd3 = Tn(G["reset_u_dof"]), Tn(G["reset_u_cmd"])
    reset_extra = (Tn(G["reset_u_xy"]), Tn(G["reset_r_level"])) if generic else ()
    if generic:
        # what the generator planted between the warm-up and reset_idx: the listed envs' tracking sums, the pre-reset base positions
        if hip:
            env.buf.view("episode_sums")[:, TRACKING] = Tn(G["plant_tracking_lin_vel"]).to(env.dev)
            env.buf.root.copy_(Tn(G["plant_root"]))
        else:
            o.episode_sums[:, TRACKING] = Tn(G["plant_tracking_lin_vel"])
            o.sim.root[:] = Tn(G["plant_root"])
    if hip:
        before = RC.snapshot(env.buf)
        RC.reset_idx_call(env, G["ids"], u_dof, u_cmd3, *reset_extra)
        RC.check_untouched(env.buf, before, m, "reset_idx")
        b = env.buf
        got = dict((name, b.view(name)) for name in AFTER_FIELDS)
        got.update(reset=b.reset, ep_len=b.episode_length, extras_time_outs=b.extras_time_outs, extras_episode=b.extras_episode,
                   root=b.root, dof=b.dof_state, base_euler=b.view("base_euler"))
        hist = (b.obs_ring.abs().amax(dim=(1, 2)), b.priv_ring.abs().amax(dim=(1, 2)))
        if generic:
            _check_generic(b.terrain_levels, b.view("env_origins"), b.measured_heights, b.command_range_x.cpu(),
                           lambda k: G["after_" + k], "after reset_idx:")
    else:
        o._reset_masked(m, u_dof, u_cmd3, *reset_extra)
        got = dict((name, getattr(o, name)) for name in AFTER_FIELDS)
        got.update(reset=o.reset, ep_len=o.ep_len, extras_time_outs=o.extras_time_outs, extras_episode=o.extras_episode, root=o.sim.root,
                   dof=torch.stack((o.sim.dof_pos, o.sim.dof_vel), -1).view(-1, 2), base_euler=o.base_euler)
        hist = (o.obs_hist.abs().amax(dim=(1, 2)), o.priv_hist.abs().amax(dim=(1, 2)))
        if generic:
            _check_generic(o.terrain.levels, o.env_origins, o.measured_heights, o.cmd_range_x, lambda k: G["after_" + k], "after reset_idx:")
    for k in ("reset", "ep_len", "extras_time_outs"):
        EC.exact(got[k], G["after_" + k], "after reset_idx: " + k)
    for k in AFTER_FIELDS + ("root", "dof"):
        EC.close(got[k], G["after_" + k], "after reset_idx: " + k)
    EC.close(got["base_euler"][m.to(got["base_euler"].device)], G["after_base_euler"][m.numpy()], "after reset_idx: base_euler (listed)")
    EC.close(got["extras_episode"], G["after_extras_episode"], "after reset_idx: extras episode", rtol=1e-5, atol=1e-7)
    for h, name in zip(hist, ("obs_history", "critic_history")):
        assert float(h[m.to(h.device)].abs().max()) == 0.0 and float(G["after_" + name][m.numpy()].max()) == 0.0, name
    if generic:                       # the command curriculum was decided inside the partial reset, on the listed envs
        assert [float(v) for v in G["after_cmd_range_x"]] != [float(v) for v in G["warm_cmd_range_x"][-1]]
    for t in range(G["step_rew"].shape[0]):
        step(lambda k, t=t: G["step_" + k][t], "step %d after reset_idx" % t)
    assert bool(G["step_reset"][0][4])          # a listed env reset again by the step kernel's own mask
