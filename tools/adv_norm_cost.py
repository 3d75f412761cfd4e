"""What PPO.advantage_normalization costs at the training script's size (profiles/adv_norm_modes_cost.txt).

  modes   the three modes -- batch, minibatch, none -- as three runners in one process, legs alternating; per leg the update's time (the
          runner's HIP events around it), the rollout's, and env-steps/s over learn(iters) by a host clock around a device synchronise.
  call    hgym_adv_normalize_minibatches on its own at the same shape (T N entries in num_mini_batches segments over a random
          permutation): HIP events around each call, the median of 30, its bytes (indices read twice, the column gathered twice, the
          second column scattered once) over that time, next to a device-to-device copy of as many bytes timed the same way.

python tools/adv_norm_cost.py [num_envs] [iters] [legs]"""
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
MODES = ("batch", "minibatch", "none")


def _runner(num_envs, mode):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    if mode != "batch":
        train_cfg.algorithm.advantage_normalization = mode
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    assert runner.alg._adv_mode == mode and (runner.alg.storage.advantages_mb is not None) == (mode == "minibatch")
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
    out["graphs"] = {m: r._update_graph is not None for m, r in runners.items()}
    alg = runners["minibatch"].alg
    out["shape"] = dict(rows=int(alg.storage.advantages_mb.numel()), segments=int(alg.num_mini_batches),
                        seg_len=int(alg.storage.advantages_mb.numel()) // int(alg.num_mini_batches))
    return out


def _median_us(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return dict(median_us=times[len(times) // 2], min_us=times[0], max_us=times[-1])


def call_cost(rows, segments):
    import hgym
    from hgym import _lib as L
    seg_len = rows // segments
    g = torch.Generator(device="cuda").manual_seed(3)
    adv = torch.randn(rows, device="cuda", generator=g)
    out = torch.zeros(rows, device="cuda")
    idx = torch.randperm(rows, device="cuda", generator=g)[:segments * seg_len].contiguous()
    scratch = L.adv_mb_scratch(segments, seg_len, "cuda")
    nbytes = 2 * idx.numel() * 8 + 2 * idx.numel() * 4 + idx.numel() * 4      # idx twice, adv gathered twice, out scattered
    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")      # a copy reads and writes
    call = _median_us(lambda: hgym.adv_normalize_minibatches(idx, adv, out, segments, scratch))
    copy_ = _median_us(lambda: dst.copy_(src))
    for d in (call, copy_):
        d["gb_per_s"] = nbytes / d["median_us"] / 1e3
    return dict(rows=rows, segments=segments, seg_len=seg_len, bytes=nbytes, call=call, device_copy_of_the_same_bytes=copy_)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "adv_norm_cost.py measures on the GPU; none visible"
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    modes = modes_cost(n, iters, legs)
    print(json.dumps(dict(modes=modes, call=call_cost(modes["shape"]["rows"], modes["shape"]["segments"])), indent=1), flush=True)
