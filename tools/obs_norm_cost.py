"""Empirical observation normalisation, what it costs (profiles/empirical_normalization_cost.txt): iteration time with the feature on
against off, two runners alternating in one process; the accumulate launch against a device-to-device copy of the same bytes; the small
launches (medians of 30 by HIP events); the largest |m| s over the columns after the iterations run here.  Prints one JSON document."""
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "humanoid-gym_amd"))
import numpy as np
import torch

OBS = [("command_input", 5), ("q", 12), ("dq", 12), ("actions", 12), ("base_ang_vel", 3), ("base_euler", 3)]
PRIV = [("command_input", 5), ("dof_pos", 12), ("dof_vel", 12), ("actions", 12), ("diff", 12), ("base_lin_vel", 3), ("base_ang_vel", 3),
        ("base_euler", 3), ("push_force", 2), ("push_torque", 3), ("friction", 1), ("mass/30", 1), ("stance_mask", 2), ("contact_mask", 2)]


def name(c, table, width):
    f, k = divmod(c, width)
    for n, w in table:
        if k < w:
            return "frame %d %s[%d]" % (f, n, k)
        k -= w


def runner(norm, N=4096):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(N), "--seed", "1"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="humanoid_ppo"))
    if norm:
        train_cfg.policy.empirical_normalization = True
    env, _ = task_registry.make_env(name="humanoid_ppo", args=args, env_cfg=env_cfg)
    r, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    return r


def timed(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return dict(median_us=t[len(t) // 2], min_us=t[0], max_us=t[-1], reps=reps)


def main():
    out = {}
    off, on = runner(False), runner(True)
    for r in (off, on):
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)      # eager, capture, replays
    legs = {"off": [], "on": []}
    for rnd in range(4):
        for tag, r in (("off", off), ("on", on)):
            r.learn(num_learning_iterations=10, init_at_random_ep_len=False)
            ms = r.last_iteration_ms[1:]
            legs[tag].append(statistics.median(ms))
    out["iteration_ms"] = {k: dict(medians_per_leg=v, median=statistics.median(v)) for k, v in legs.items()}
    out["update_graph"] = dict(off=off._update_graph is not None, on=on._update_graph is not None)
    alg, net, st = on.alg, on.alg.net, on.alg.storage
    T, N = st.num_transitions_per_env, st.num_envs
    obs, priv = st._obs_all[:T].flatten(0, 1), st._priv_all[:T].flatten(0, 1)
    nbytes = obs.numel() * 4 + priv.numel() * 4
    keep = [net.norm_view(n, k).clone() for k in (0, 1) for n in ("mean", "var")] + [net.norm_view("header").clone()]
    a = timed(lambda: net.norm_accumulate(obs, priv))
    d_obs, d_priv = torch.empty_like(obs), torch.empty_like(priv)
    c = timed(lambda: (d_obs.copy_(obs), d_priv.copy_(priv)))
    out["accumulate"] = dict(rows=T * N, bytes_read=nbytes, **a, read_GBps=nbytes / a["median_us"] * 1e-3,
                             copy=dict(**c, bytes_read=nbytes, bytes_written=nbytes, read_GBps=nbytes / c["median_us"] * 1e-3,
                                       read_plus_write_GBps=2 * nbytes / c["median_us"] * 1e-3))
    out["unfold"] = timed(lambda: net.norm_unfold_grad())
    net.norm_view("sums").zero_()
    out["merge_refold_empty_batch"] = timed(lambda: net.norm_merge())
    out["sync_shadow_with_fold"] = timed(lambda: net.sync_shadow())
    out["sync_shadow_plain_net"] = timed(lambda: off.alg.net.sync_shadow())
    torch.cuda.synchronize()
    # the largest |m| s
    for k, (table, width, tag) in enumerate(((OBS, 47, "obs"), (PRIV, 73, "critic_obs"))):
        m, s = net.norm_view("mean_f", k).cpu().numpy().astype(np.float64), net.norm_view("scale_f", k).cpu().numpy().astype(np.float64)
        ms = np.abs(m) * s
        top = np.argsort(-ms)[:8]
        out["abs_mean_times_scale_" + tag] = dict(count=float(net.norm_view("header")[2 + k]), max=float(ms.max()),
                                                  top=[dict(col=int(c), name=name(int(c), table, width), m=float(m[c]), s=float(s[c]),
                                                            m_s=float(ms[c])) for c in top],
                                                  columns_above_8=int((ms > 8).sum()), columns_above_1=int((ms > 1).sum()), columns=int(ms.size))
    # hgym_ppo_apply: norm-squared pass + Adam + bias fold (on) against prologue + Adam (off); moves the parameters, so last
    out["ppo_apply_on"] = timed(lambda: net.ppo_apply(alg._ppo_cfg))
    out["ppo_apply_off"] = timed(lambda: off.alg.net.ppo_apply(off.alg._ppo_cfg))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
