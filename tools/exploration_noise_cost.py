"""What PPO.exploration_noise costs at the training script's size (profiles/exploration_noise_cost.txt).  Cost only: the effect on a
learning curve is not measured here.

One process, PPO runners (humanoid_ppo) at num_envs x 60 steps: the option off, {"kind": "colored", "beta": 0.5} and {"kind": "ar1", "rho": 0.9}.

  table    HIP events around hgym_policy_noise_table alone (ExplorationNoise.fill on the runner's own buffers), the median of `reps`, beside
           a device-to-device copy of the table's bytes (the floor for writing them once) -- and, from the loops, one rollout.
  loops    learn(iters) of the runners, legs alternating, rollout and update graphs captured: ms per iteration by a host clock around a
           device synchronise, and the runner's own split into rollout and update.

Writes sections 1 and 2 of the profile to `out` (default profiles/exploration_noise_cost.txt) and prints the raw record as JSON.  Section
3 of the profile -- bench.py with the option off against the parent commit -- is two checkouts alternating (bench.py --gpus 1
--no-cpu-baseline --no-roofline --configs none in each), not this script: its lines are appended to the file by hand.

python tools/exploration_noise_cost.py [num_envs] [iters] [legs] [reps] [out]"""
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

FILTERS = dict(off=None, colored={"kind": "colored", "beta": 0.5}, ar1={"kind": "ar1", "rho": 0.9})


def _runner(num_envs, noise):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="humanoid_ppo"))
    if noise is not None:
        train_cfg.algorithm.exploration_noise_cfg = noise
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    return runner


def _median_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out), reps=reps)


def table_cost(runners, reps):
    out = {}
    with torch.inference_mode():
        for name, r in runners.items():
            noise = r.alg._noise
            if noise is None:
                continue
            step, seed = r.alg._sample_step.clone(), r.alg.actor_critic._sample_seed
            keep = None if noise.state is None else noise.state.clone()      # (the timed calls move the AR(1) state on: put back below)
            out[name] = _median_us(lambda: noise.fill(step, seed), reps)
            out[name].update(table_bytes=noise.table.numel() * 4, shape=list(noise.table.shape))
            if keep is not None:
                noise.state.copy_(keep)
            if "copy" not in out:
                dst = torch.empty_like(noise.table)
                out["copy"] = _median_us(lambda: dst.copy_(noise.table), reps)
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
    out["plans"] = {m: dict(rollout_graph=r._graph is not None, update_graph=r._update_graph is not None,
                            fuse=r.env.rollout_fused_mode(r.alg.net)) for m, r in runners.items()}
    return out


def report(res):
    """Sections 1 and 2 of profiles/exploration_noise_cost.txt from the record."""
    n, T, tb, lp = res["num_envs"], res["steps"], res["table"], res["loops"]
    mean = lambda m, k: statistics.mean(leg[k] for leg in lp[m])
    span = lambda m, k: (min(leg[k] for leg in lp[m]), max(leg[k] for leg in lp[m]))
    out = ["PPO.exploration_noise: what the option costs at %d envs x %d steps (tools/exploration_noise_cost.py; DESIGN.md section 35)" % (n, T),
           "Cost only: the effect on a learning curve is not measured.", "",
           "1. hgym_policy_noise_table on its own: HIP events around one call, the median of %d (min .. max), microseconds" % tb["copy"]["reps"]]
    for m in ("colored", "ar1"):
        out.append("   %-8s table (%s, %.1f MB): %7.1f us  (%.1f .. %.1f)" % (m, " x ".join(str(v) for v in tb[m]["shape"]), tb[m]["table_bytes"] / 1e6,
                                                                         tb[m]["median_us"], tb[m]["min_us"], tb[m]["max_us"]))
    out.append("   device copy of as many bytes:       %7.1f us  (%.1f .. %.1f)" % (tb["copy"]["median_us"], tb["copy"]["min_us"], tb["copy"]["max_us"]))
    out.append("   one rollout with the option off:    %7.1f us  (the mean of section 2's legs)" % (mean("off", "rollout_ms") * 1e3))
    out += ["", "2. An iteration with the option off and on: %d runners alternating in one process, %d legs of %d iterations each, rollout and update" % (
        len(FILTERS), res["legs"], res["iters"]), "   graphs captured (%s); ms per iteration by a host clock around a device synchronise, rollout / update the runner's own split" % (
        ", ".join("%s: %s" % (m, "rollout %s, update graph %s" % (p["fuse"], p["update_graph"])) for m, p in lp["plans"].items()))]
    for m in FILTERS:
        for i, leg in enumerate(lp[m]):
            out.append("   %-8s leg %d: %.3f ms/iter  %.2f M env-steps/s  rollout %.3f  update %.3f" % (m, i + 1, leg["ms_per_iteration"],
                                                                                                  leg["env_steps_per_s"] / 1e6, leg["rollout_ms"], leg["update_ms"]))
    lo, hi = span("off", "rollout_ms")
    out.append("   means: " + "; ".join("%s %.3f ms/iter, rollout %.3f, update %.3f" % (m, mean(m, "ms_per_iteration"), mean(m, "rollout_ms"),
                                                                                mean(m, "update_ms")) for m in FILTERS))
    out.append("   the off-legs' own rollout spread: %.3f .. %.3f ms (%.1f us)" % (lo, hi, (hi - lo) * 1e3))
    for m in ("colored", "ar1"):
        d = (mean(m, "rollout_ms") - mean("off", "rollout_ms")) * 1e3
        out.append("   %-8s rollout - off rollout = %+.1f us; the table launch alone is %.1f us, so the %d launches of the rollout itself move by %+.1f us"
                   % (m, d, tb[m]["median_us"], T, d - tb[m]["median_us"]))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    assert torch.cuda.is_available(), "exploration_noise_cost.py measures on the GPU; none visible"
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 4096
    iters = int(argv[1]) if len(argv) > 1 else 20
    legs = int(argv[2]) if len(argv) > 2 else 3
    reps = int(argv[3]) if len(argv) > 3 else 30
    runners = {name: _runner(n, cfg) for name, cfg in FILTERS.items()}
    for r in runners.values():
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)        # eager, capture, replays
    torch.cuda.synchronize()
    res = dict(num_envs=n, steps=runners["off"].num_steps_per_env, iters=iters, legs=legs,
               lag1={m: (None if r.alg._noise is None else r.alg._noise.lag1) for m, r in runners.items()},
               loops=loops_cost(runners, n, iters, legs))
    res["table"] = table_cost(runners, reps)
    path = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "exploration_noise_cost.txt")
    with open(path, "w") as f:
        f.write(report(res))
    print(json.dumps(res, indent=1), flush=True)
