"""What PPO.diagnostics() costs: python tools/ppo_diagnostics_cost.py [num_envs] [iters] [legs] [--once]

  * one PPO.diagnostics(sync=False) behind a real update at train.py's default configuration (num_envs x 60 steps): HIP events around
    the call, median of 30;
  * the reduction alone (hgym_ppo_diag_reduce over the same rows) next to a device copy of the same number of bytes, same process;
  * train.py's default throughput (logging on) with runner.diag_interval = 0 and 10, legs alternating in one process.
--once: one iteration and ONE diagnostics call, nothing timed -- the run to put under `rocprofv3 --kernel-trace --stats` for the
split between the two forwards and the reduction."""
import contextlib
import copy
import ctypes as C
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "humanoid-gym_amd")]

import torch  # noqa: E402

from humanoid.envs import task_registry  # noqa: E402
from humanoid.utils import get_args  # noqa: E402

BYTES_PER_ROW = 4 * 48 + 5 * 4      # four (M, 12) columns + five (M,) columns, fp32


def make(num_envs, root, interval=0):
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=args.task))
    train_cfg.runner.diag_interval = interval
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=root)
    return runner


def timed(fn, n=30):
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def one_call(num_envs, once):
    from hgym import _lib as L
    with contextlib.redirect_stdout(io.StringIO()):
        r = make(num_envs, None, interval=1)            # learn() prepares and runs the pass: the storage is left ready for more calls
        r.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    alg = r.alg
    if once:
        alg.diagnostics(sync=False)
        torch.cuda.synchronize()
        return
    alg.diagnostics(sync=False)
    med, lo, hi = timed(lambda: alg.diagnostics(sync=False))
    st = alg.storage
    M = st.num_transitions_per_env * st.num_envs
    print(json.dumps(dict(what="PPO.diagnostics(sync=False)", rows=M, median_ms=med, min_ms=lo, max_ms=hi, last=alg.diagnostics())), flush=True)
    # the reduction alone, against a copy of the same bytes
    fl = lambda t: t.flatten(0, 1)
    mu_new, v_new = torch.randn(M, 12, device="cuda") * 0.1 + fl(st.mu), st.values.view(-1) + 0.01
    cols = [fl(st.actions), fl(st.mu), fl(st.sigma), mu_new, st.actions_log_prob.view(-1), st.values.view(-1), st.returns.view(-1),
            st.advantages.view(-1), v_new]
    block = L.diag_block(M, "cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reduce():
        L.check(L.lib.hgym_ppo_diag_reduce(M, *[L.fptr(t) for t in cols], L.fptr(alg.net.params), 0.2, 0, M, 1, L.f64ptr(block), s))
    src = torch.empty(M * BYTES_PER_ROW // 2, dtype=torch.uint8, device="cuda")        # a copy reads and writes: half the bytes each way
    dst = torch.empty_like(src)
    reduce(), dst.copy_(src)
    rm, cm = timed(reduce), timed(lambda: dst.copy_(src))
    nbytes = M * BYTES_PER_ROW
    print(json.dumps(dict(what="hgym_ppo_diag_reduce (+ finish launch) vs device copy moving the same bytes", bytes=nbytes,
                          reduce_median_ms=rm[0], reduce_GBps=nbytes / rm[0] * 1e-6, copy_median_ms=cm[0], copy_GBps=nbytes / cm[0] * 1e-6)),
          flush=True)


def leg(num_envs, iters, interval, root):
    with contextlib.redirect_stdout(io.StringIO()):
        runner = make(num_envs, root, interval)
        runner.learn(num_learning_iterations=5, init_at_random_ep_len=True)
        runner.wait_for_saves()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.learn(num_learning_iterations=iters, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        runner.wait_for_saves()
    return dict(diag_interval=interval, env_steps_per_s=runner.num_steps_per_env * num_envs * iters / dt,
                last_diag_iteration=runner.last_diag_iteration)


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    num_envs = int(argv[0]) if len(argv) > 0 else 4096
    iters = int(argv[1]) if len(argv) > 1 else 200
    legs = int(argv[2]) if len(argv) > 2 else 3
    one_call(num_envs, "--once" in sys.argv)
    if "--once" not in sys.argv:
        with tempfile.TemporaryDirectory() as tmp:
            for k in range(2 * legs):
                print(json.dumps(leg(num_envs, iters, 10 if (k & 1) else 0, os.path.join(tmp, "leg%d" % k))), flush=True)
