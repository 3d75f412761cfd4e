"""What left-right symmetry augmentation (PPO.symmetry) costs at the training script's size (profiles/symmetry_augmentation_cost.txt).

  1. RolloutStorage.mirror() alone on a 4096-env x 60-step storage with valid shadows: median of `reps` runs by HIP events, the bytes it
     reads and writes computed from the shapes, and a device-to-device copy of the same byte count timed the same way in this process.
  2. Iteration time with symmetry on against off: two runners in one process, legs alternating; env-steps/s over learn(iters) by a host
     clock around a device synchronise, and the runner's own rollout / update split (HIP events).

python tools/symmetry_cost.py [num_envs] [iters] [legs] [reps]"""
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "humanoid-gym_amd"))

import torch  # noqa: E402

TASK = "humanoid_ppo"


def _median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def mirror_cost(num_envs, T, reps):
    from humanoid.envs import task_registry      # noqa: F401
    from humanoid.utils import task_registry as reg
    from humanoid.utils.symmetry import xbot_l_mirror
    from humanoid.algo.ppo.rollout_storage import RolloutStorage
    spec = xbot_l_mirror(reg.get_cfgs(TASK)[0])
    st = RolloutStorage(num_envs, T, [705], [219], [12], "cuda")
    st.enable_mirror(spec)
    st.enable_shadow(768, 256)
    st._obs_store.normal_()
    st._priv_store.normal_()
    st.shadow_valid = [True] * T
    rows = T * num_envs
    # read + written bytes: fp32 obs / priv rows, three 12-wide columns, four scalar columns, the two shadows (their whole padded rows are written, 705 / 219 columns of them read)
    nbytes = rows * (2 * 4 * (705 + 219 + 3 * 12 + 4) + 2 * (705 + 768 + 219 + 256))
    m = _median_ms(st.mirror, reps)
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    c = _median_ms(lambda: b.copy_(a), reps)
    return dict(rows=rows, bytes=nbytes, mirror_ms=dict(median=m[0], min=m[1], max=m[2]), mirror_GBps=nbytes / m[0] * 1e-6,
                copy_ms=dict(median=c[0], min=c[1], max=c[2]), copy_GBps=nbytes / c[0] * 1e-6, launches_per_mirror=7 + 4)


def _runner(num_envs, symmetry):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    if symmetry:
        train_cfg.algorithm.symmetry = True
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    return runner


def iteration_cost(num_envs, iters, legs):
    runners = {False: _runner(num_envs, False), True: _runner(num_envs, True)}
    for r in runners.values():
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)        # eager, capture, replays
    torch.cuda.synchronize()
    out = {False: [], True: []}
    for _ in range(legs):
        for on in (False, True):
            r = runners[on]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.learn(num_learning_iterations=iters, init_at_random_ep_len=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[on].append(dict(ms_per_iteration=dt / iters * 1e3, env_steps_per_s=r.num_steps_per_env * num_envs * iters / dt,
                                rollout_ms=r.last_collection_time * 1e3, update_ms=r.last_learn_time * 1e3))
    return dict(off=out[False], on=out[True], minibatch_rows=dict(off=int(runners[False].alg.net.cfg.max_batch), on=int(runners[True].alg.net.cfg.max_batch)))


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
    assert torch.cuda.is_available(), "symmetry_cost.py measures on the GPU; none visible"
    print(json.dumps(dict(mirror=mirror_cost(n, 60, reps)), indent=1), flush=True)
    print(json.dumps(dict(iteration=iteration_cost(n, iters, legs)), indent=1), flush=True)
