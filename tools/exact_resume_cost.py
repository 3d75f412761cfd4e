"""What `exact_resume` costs a logging run: train.py's default configuration (4096 envs, logging on, a checkpoint every 100 iterations)
with and without the env-state sidecar, alternating in one process.  Per leg: env-steps/s over learn(ITERS) and the training thread's
host time per checkpoint (OnPolicyRunner.save_time_s).  python tools/exact_resume_cost.py [num_envs] [iters] [legs]"""
import contextlib
import copy
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "humanoid-gym_amd")]

import torch  # noqa: E402

from humanoid.envs import task_registry  # noqa: E402
from humanoid.utils import get_args  # noqa: E402


def leg(num_envs, iters, exact, root):
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=args.task))
    if exact:
        train_cfg.runner.exact_resume = True
    with contextlib.redirect_stdout(io.StringIO()):
        env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
        runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=root)
        runner.learn(num_learning_iterations=5, init_at_random_ep_len=True)          # eager, capture, replay; the process's first torch.save
        runner.wait_for_saves()
        torch.cuda.synchronize()
        saves0, t0 = runner.save_time_s, time.perf_counter()
        runner.learn(num_learning_iterations=iters, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        host = runner.save_time_s - saves0
        t1 = time.perf_counter()
        runner.wait_for_saves()
        wait = time.perf_counter() - t1
    n_ckpt = len([it for it in range(5, 5 + iters) if it % runner.save_interval == 0]) + 1
    side = [f for f in os.listdir(runner.log_dir) if f.startswith("envstate")]
    size = max((os.path.getsize(os.path.join(runner.log_dir, f)) for f in side), default=0)
    return dict(exact_resume=exact, env_steps_per_s=runner.num_steps_per_env * num_envs * iters / dt, checkpoints=n_ckpt,
                save_time_ms_per_checkpoint=host / n_ckpt * 1e3, writer_wait_ms=wait * 1e3, sidecar_bytes=size)


if __name__ == "__main__":
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(2 * legs):
            print(json.dumps(leg(num_envs, iters, bool(k & 1), os.path.join(tmp, "leg%d" % k))), flush=True)
