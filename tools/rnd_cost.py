"""What Random Network Distillation (PPO.rnd, hgym_rnd_rewards) costs at the training script's size (profiles/rnd_cost.txt).

One process, two PPO runners (humanoid_ppo) side by side at num_envs x 60 steps, one without and one with rnd_cfg (the default
dimensions, a constant weight):

  loops    learn(iters) of either runner, legs alternating: ms per iteration by a host clock around a device synchronise, and the runner's own
           split into rollout and update.
  calls    HIP events around eager calls on the rows the last rollout left, medians over `reps`: hgym_rnd_rewards alone (three launches),
           a device-to-device copy of as many bytes as it moves beside it, the whole reward pass (state copy, the two forwards, the
           kernel) and one predictor step (hgym_bc_grad + hgym_ppo_apply).

python tools/rnd_cost.py [num_envs] [iters] [legs] [reps]"""
import copy
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "humanoid-gym_amd"))

import torch  # noqa: E402


def _runner(num_envs, rnd):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="humanoid_ppo"))
    if rnd is not None:
        train_cfg.algorithm.rnd_cfg = rnd
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    return runner


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), reps=reps)


def calls_cost(runner, reps):
    from hgym import _lib as L
    alg, st, rnd = runner.alg, runner.alg.storage, runner.alg._rnd
    T, N, K = st.num_transitions_per_env, st.num_envs, rnd.num_outputs
    out = dict(T=T, N=N, K=K, S=rnd.num_states)
    block = L.rnd_block(N, st.rewards.device)      # a block of its own: the run's statistics are left alone
    rewards = st.rewards.clone()
    s = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        L.check(L.lib.hgym_rnd_rewards(T, N, K, L.fptr(st.rnd_pred), L.fptr(st.rnd_target[1:]), L.fptr(rewards), L.fptr(st.rnd_error),
                                       L.fptr(st.rnd_intrinsic), C.byref(rnd.rnd_cfg), L.f64ptr(block), s()), "hgym_rnd_rewards")
    out["rnd_rewards"] = _median_ms(kernel, reps)
    # both embeddings read; err written, read twice; rewards read and written; intrinsic written
    nbytes = 4.0 * T * N * (2 * K + 6)
    out["rnd_rewards"]["bytes"] = nbytes
    out["rnd_rewards"]["gbytes_per_s"] = nbytes / (out["rnd_rewards"]["median_ms"] * 1e-3) / 1e9
    src = torch.empty(int(nbytes) // 2, dtype=torch.uint8, device=st.rewards.device)      # a copy MOVES twice its size: read + write
    dst = torch.empty_like(src)
    out["copy_same_bytes"] = _median_ms(lambda: dst.copy_(src), reps)
    out["copy_same_bytes"]["bytes"] = 2.0 * src.numel()
    out["ratio_to_copy"] = out["rnd_rewards"]["median_ms"] / out["copy_same_bytes"]["median_ms"]
    keep = rnd.block.clone()

    def whole():
        rnd.reward_pass(st)
    out["reward_pass"] = _median_ms(whole, reps)
    rnd.block.copy_(keep)
    idx = torch.arange(int(alg.net.cfg.max_batch), dtype=torch.int64, device=st.rewards.device)
    out["predictor_step"] = _median_ms(lambda: rnd.train_step(st, idx), reps)
    out["predictor_step"]["rows"] = int(idx.numel())
    return out


def loops_cost(runners, num_envs, iters, legs):
    out = {m: [] for m in runners}
    for _ in range(legs):
        for m, r in runners.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.learn(num_learning_iterations=iters, init_at_random_ep_len=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[m].append(dict(ms_per_iteration=dt / iters * 1e3, env_steps_per_s=r.num_steps_per_env * num_envs * iters / dt,
                               rollout_ms=r.last_collection_time * 1e3, update_ms=r.last_learn_time * 1e3))
    out["plans"] = {m: dict(rollout_graph=r._graph is not None, update_graph=r._update_graph is not None) for m, r in runners.items()}
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "rnd_cost.py measures on the GPU; none visible"
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 4096
    iters = int(argv[1]) if len(argv) > 1 else 20
    legs = int(argv[2]) if len(argv) > 2 else 3
    reps = int(argv[3]) if len(argv) > 3 else 30
    runners = dict(off=_runner(n, None), rnd=_runner(n, dict(weight=1.0)))
    for r in runners.values():
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)        # eager, capture, replays
    torch.cuda.synchronize()
    res = dict(num_envs=n, loops=loops_cost(runners, n, iters, legs))
    res["calls"] = calls_cost(runners["rnd"], reps)
    res["rnd_log"] = runners["rnd"].alg._rnd.read_log(runners["rnd"].alg._log.split(runners["rnd"].alg.log_block().cpu()))
    print(json.dumps(res, indent=1), flush=True)
