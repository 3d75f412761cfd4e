"""What PPO.value_normalization costs at the training script's size (profiles/value_normalization_cost.txt).

  runs    three runners in one process, legs alternating, both graphs captured: the option off, the option off with the deferred critic
          (HGYM_ROLLOUT_CRITIC=deferred around that runner's learn() calls: the one-launch rollout's other form, which the option takes),
          the option on; per leg the iteration's time (host clock around a device synchronise), the rollout's and the update's (the
          runner's HIP events).
  calls   the three entry points on their own at the same shape (T N values): HIP events around each eager call, the median of 30, next
          to a device-to-device copy of the same bytes timed the same way.

python tools/value_norm_cost.py [num_envs] [iters] [legs]"""
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
RUNS = ("off", "off-deferred", "on")


def _runner(num_envs, on):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    if on:
        train_cfg.algorithm.value_normalization = True
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    assert (runner.alg.value_normalizer is not None) == on
    return runner


def _learn(name, runner, iters, first=False):
    if name == "off-deferred":
        os.environ["HGYM_ROLLOUT_CRITIC"] = "deferred"
    try:
        runner.learn(num_learning_iterations=iters, init_at_random_ep_len=first)
    finally:
        os.environ.pop("HGYM_ROLLOUT_CRITIC", None)


def runs_cost(num_envs, iters, legs):
    from humanoid.algo.ppo.on_policy_runner import _plan_loop
    runners = {name: _runner(num_envs, name == "on") for name in RUNS}
    for name, r in runners.items():
        _learn(name, r, 4, first=True)        # eager, capture, replays
    torch.cuda.synchronize()
    out = {name: [] for name in RUNS}
    for _ in range(legs):
        for name, r in runners.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _learn(name, r, iters)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[name].append(dict(ms_per_iteration=dt / iters * 1e3, env_steps_per_s=r.num_steps_per_env * num_envs * iters / dt,
                                  rollout_ms=r.last_collection_time * 1e3, update_ms=r.last_learn_time * 1e3))
    out["graphs"] = {name: (r._graph is not None, r._update_graph is not None) for name, r in runners.items()}
    out["fuse"] = {name: _plan_loop(r.env, r.alg, r.device, False).fuse for name, r in runners.items()}
    out["fuse"]["off-deferred"] = "deferred (HGYM_ROLLOUT_CRITIC)"
    st = runners["on"].alg.storage
    out["shape"] = dict(values=int(st.returns.numel()), block=[float(x) for x in runners["on"].alg.value_normalizer.block.cpu()])
    return out


def _median_us(fn, reps=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return sorted(times)[len(times) // 2]


def calls_cost(n):
    import hgym
    from hgym import _lib as L
    x = torch.randn(n, device="cuda") * 2.0 + 5.0
    y, dst = x.clone(), torch.empty_like(x)
    block, scratch = L.value_norm_block("cuda"), L.value_norm_scratch(n, "cuda")
    hgym.value_norm_merge(x, block, scratch)
    return dict(values=n, bytes_read=4 * n,
                denormalize_us=_median_us(lambda: hgym.value_denormalize(x, block, 1e-2, out=dst)),
                merge_us=_median_us(lambda: hgym.value_norm_merge(x, block, scratch)),
                normalize_us=_median_us(lambda: hgym.value_normalize(y, block, 1e-2)),
                copy_us=_median_us(lambda: dst.copy_(x)))


if __name__ == "__main__":
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    runs = runs_cost(num_envs, iters, legs)
    print(json.dumps(dict(num_envs=num_envs, iters=iters, legs=legs, runs=runs, calls=calls_cost(runs["shape"]["values"])), indent=1))
