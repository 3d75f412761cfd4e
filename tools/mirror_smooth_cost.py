"""What the mirror loss and the smoothness regulariser cost TOGETHER at the training script's size (profiles/mirror_smooth_cost.txt).

  default   four modes -- neither option, the mirror loss alone (no augmentation), smoothness alone (both terms), the combination -- as
            four runners in one process, legs alternating; per leg the update's time (the runner's HIP events around it), the
            rollout's, and ms per iteration over learn(iters) by a host clock around a device synchronise.  Both HIP graphs are
            captured in the warm-up.  The summary holds the means and the combined update against the sum of the two increments.
  --trace   one runner in one mode (default: the combination), a few iterations and nothing else: the process to put under
            `rocprofv3 --kernel-trace --stats` for the per-launch figures (mlp_fb_head_kernel<FbMirrorSmooth, ..> beside
            mlp_fb_head_kernel<FbSmooth, ..> of a `smooth` trace from the same box).

python tools/mirror_smooth_cost.py [num_envs] [iters] [legs]      |      python tools/mirror_smooth_cost.py --trace [num_envs] [iters] [off|mirror|smooth|both]"""
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "humanoid-gym_amd"))

import torch  # noqa: E402

TASK = "humanoid_ppo"
SMOOTH = dict(temporal_coef=1.0, spatial_coef=1.0)
MODES = dict(off=(0.0, None), mirror=(0.5, None), smooth=(0.0, SMOOTH), both=(0.5, SMOOTH))      # (mirror_loss_coef, smoothness_cfg)


def _runner(num_envs, mode):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    coef, smooth = MODES[mode]
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    if smooth is not None:
        train_cfg.algorithm.smoothness_cfg = dict(smooth)
    if coef:
        train_cfg.algorithm.mirror_loss_coef = coef      # (no `symmetry`: the tables without the augmentation)
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    alg = runner.alg
    assert (alg._smooth is not None) == (smooth is not None) and (alg._mirror_loss is not None) == bool(coef) and not alg._augment
    return runner


def modes_cost(num_envs, iters, legs):
    runners = {m: _runner(num_envs, m) for m in MODES}
    for r in runners.values():
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)        # eager, capture, replays
    torch.cuda.synchronize()
    out = {m: [] for m in MODES}
    for _ in range(legs):
        for m, r in runners.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.learn(num_learning_iterations=iters, init_at_random_ep_len=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[m].append(dict(ms_per_iteration=dt / iters * 1e3, env_steps_per_s=r.num_steps_per_env * num_envs * iters / dt,
                               rollout_ms=r.last_collection_time * 1e3, update_ms=r.last_learn_time * 1e3))
    mean = lambda m, k: sum(leg[k] for leg in out[m]) / len(out[m])
    upd = {m: mean(m, "update_ms") for m in MODES}
    out["summary"] = dict(update_ms=upd, ms_per_iteration={m: mean(m, "ms_per_iteration") for m in MODES},
                          increment_mirror_ms=upd["mirror"] - upd["off"], increment_smooth_ms=upd["smooth"] - upd["off"],
                          increment_both_ms=upd["both"] - upd["off"],
                          both_minus_sum_of_increments_ms=(upd["both"] - upd["off"]) - (upd["mirror"] - upd["off"]) - (upd["smooth"] - upd["off"]))
    out["minibatch_rows"] = {m: int(r.alg.net.cfg.max_batch) for m, r in runners.items()}
    out["graphs"] = {m: r._update_graph is not None for m, r in runners.items()}
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "mirror_smooth_cost.py measures on the GPU; none visible"
    argv = [a for a in sys.argv[1:] if a != "--trace"]
    n = int(argv[0]) if len(argv) > 0 else 4096
    iters = int(argv[1]) if len(argv) > 1 else 20
    if "--trace" in sys.argv:
        r = _runner(n, argv[2] if len(argv) > 2 else "both")
        r.learn(num_learning_iterations=iters, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        alg = r.alg
        print(json.dumps(dict(trace=dict(iterations=iters, minibatches=iters * alg.num_learning_epochs * alg.num_mini_batches,
                                         minibatch_rows=int(alg.net.cfg.max_batch)))), flush=True)
    else:
        legs = int(argv[2]) if len(argv) > 2 else 3
        print(json.dumps(dict(modes=modes_cost(n, iters, legs)), indent=1), flush=True)
