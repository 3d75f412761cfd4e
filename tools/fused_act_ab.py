#!/usr/bin/env python
"""A/B of HgymNetConfig.fused_activation on a training run: ms per iteration (collection, update) and env-steps/s for ReLU and Tanh
with the flag off (layer-by-layer gemm_nt_kernel path) and on (fused forward / update kernels, generic instantiation), legs alternating
in one process.

    python tools/fused_act_ab.py [--envs 4096] [--steps 60] [--iters 6] [--warmup 3] [--only relu-on]

--only <act>-<on|off> runs that one leg (what a kernel trace of a single leg wants)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "humanoid-gym_amd"))


def make_runner(num_envs, steps, activation, flag):
    import torch
    from humanoid.algo import OnPolicyRunner, PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    R = sys.modules[OnPolicyRunner.__module__]
    AC = getattr(R, "_ab_AC", None) or R.ActorCritic
    R._ab_AC = AC
    R.ActorCritic = lambda *a, **k: AC(*a, **dict(k, activation=activation, fused_activation=flag))
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", "1"])
    task_registry.train_cfgs[args.task].runner.num_steps_per_env = steps
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    return runner


def leg(runner, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runner.learn(num_learning_iterations=iters, init_at_random_ep_len=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    import torch.nn as nn
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    acts = {"relu": nn.ReLU(), "tanh": nn.Tanh()}
    for name, act in acts.items():
        modes = [(f, "on" if f else "off") for f in (False, True)]
        if a.only:
            modes = [(f, m) for f, m in modes if a.only == "%s-%s" % (name, m)]
        if not modes:
            continue
        runners = {m: make_runner(a.envs, a.steps, act, f) for f, m in modes}
        for m, r in runners.items():
            leg(r, a.warmup)
        times = {m: [] for m in runners}
        for _ in range(a.legs):                       # legs alternating
            for m, r in runners.items():
                times[m].append(leg(r, a.iters))
        for m, r in runners.items():
            best = min(times[m])
            print(json.dumps(dict(activation=name, fused_activation=m, fused_layout=r.alg.net.shadow_ld(0) > 0, envs=a.envs, steps=a.steps,
                                  ms_per_iteration=[round(1e3 * t, 3) for t in times[m]], env_steps_per_s=round(a.envs * a.steps / best, 1),
                                  last_collection_ms=round(1e3 * getattr(r, "last_collection_time", 0.0), 3), last_update_ms=round(1e3 * getattr(r, "last_learn_time", 0.0), 3))), flush=True)
        del runners


if __name__ == "__main__":
    main()
