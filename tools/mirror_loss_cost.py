"""What the mirror loss (PPO.mirror_loss_coef) costs at the training script's size (profiles/mirror_loss_cost.txt).

  default   the four symmetry modes -- off, augmentation alone, mirror loss alone, augmentation + mirror loss -- as four runners in one
            process, legs alternating; per leg the update's time (the runner's HIP events around it), the rollout's, and env-steps/s over
            learn(iters) by a host clock around a device synchronise.
  --trace   one runner with the mirror loss alone, a few iterations and nothing else: the process to put under
            `rocprofv3 --kernel-trace --stats` for the pre-pass's share (at 4096 envs the update's pre-pass is the only user of the
            64-row forward tiles without a finaliser, mlp_fwd_kernel<64, 16, 2, false>: its row of the kernel statistics is the pre-pass).

python tools/mirror_loss_cost.py [num_envs] [iters] [legs]      |      python tools/mirror_loss_cost.py --trace [num_envs] [iters]"""
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
COEF = 0.5
MODES = dict(off=(False, 0.0), augmentation=(True, 0.0), mirror=(False, COEF), both=(True, COEF))


def _runner(num_envs, augmentation, coef):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    if augmentation:
        train_cfg.algorithm.symmetry = True
    if coef > 0.0:
        train_cfg.algorithm.mirror_loss_coef = coef
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    alg = runner.alg
    assert alg._augment is augmentation and (alg._mirror_loss.coef if alg._mirror_loss is not None else 0.0) == coef and alg.storage.mirrored == (augmentation or coef > 0.0)
    return runner


def modes_cost(num_envs, iters, legs):
    runners = {m: _runner(num_envs, *MODES[m]) for m in MODES}
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
    out["minibatch_rows"] = {m: int(r.alg.net.cfg.max_batch) for m, r in runners.items()}
    out["graphs"] = {m: r._update_graph is not None for m, r in runners.items()}
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "mirror_loss_cost.py measures on the GPU; none visible"
    argv = [a for a in sys.argv[1:] if a != "--trace"]
    n = int(argv[0]) if len(argv) > 0 else 4096
    iters = int(argv[1]) if len(argv) > 1 else 20
    if "--trace" in sys.argv:
        r = _runner(n, *MODES["mirror"])
        r.learn(num_learning_iterations=iters, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        alg = r.alg
        print(json.dumps(dict(trace=dict(iterations=iters, prepass_launches=iters * alg.num_learning_epochs * alg.num_mini_batches,
                                         minibatch_rows=int(alg.net.cfg.max_batch)))), flush=True)
    else:
        legs = int(argv[2]) if len(argv) > 2 else 3
        print(json.dumps(dict(modes=modes_cost(n, iters, legs)), indent=1), flush=True)
