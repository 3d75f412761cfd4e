"""What PPO.guidance costs at the training script's size (profiles/guidance_cost.txt).  Cost only: the effect on XBot-L's learning curve is
not measured here.

  runs    two runners in one process, legs alternating, both graphs captured: the option off, the option on with a constant coefficient
          (the term is in every update) and a teacher of the student's widths; per leg the iteration's time (host clock around a device
          synchronise), the rollout's and the update's (the runner's HIP events).
  pass    the teacher's pass over the T N stored rows on its own (Guidance.teacher_pass: hgym_mlp_forward in pieces): HIP events around
          each eager call, the median of 30.
  tiles   one minibatch's gradient call, hgym_ppo_grad_guide beside hgym_ppo_grad on the same batch, timed the same way: the guided actor
          tiles (their own launch, the target rows staged in LDS) and the sums kernel against the plain launch.
  launch  hgym_guide_schedule on its own.

python tools/guidance_cost.py [num_envs] [iters] [legs]"""
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
RUNS = ("off", "on")


def _teacher(hidden, no, A, seed=77):
    g = torch.Generator().manual_seed(seed)
    dims, sd = [no] + list(hidden) + [A], {}
    for l in range(len(dims) - 1):
        bound = dims[l] ** -0.5
        sd["actor.%d.weight" % (2 * l)] = (torch.rand(dims[l + 1], dims[l], generator=g) * 2 - 1) * bound
        sd["actor.%d.bias" % (2 * l)] = (torch.rand(dims[l + 1], generator=g) * 2 - 1) * bound
    return sd


def _runner(num_envs, on):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    if on:
        train_cfg.algorithm.guidance_cfg = dict(coef=0.5, teacher=_teacher(train_cfg.policy.actor_hidden_dims, env_cfg.env.num_observations,
                                                                           env_cfg.env.num_actions))
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    assert (runner.alg._guide is not None) == on
    return runner


def runs_cost(num_envs, iters, legs):
    runners = {name: _runner(num_envs, name == "on") for name in RUNS}
    for r in runners.values():
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)        # eager, capture, replays
    torch.cuda.synchronize()
    out = {name: [] for name in RUNS}
    for _ in range(legs):
        for name, r in runners.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.learn(num_learning_iterations=iters, init_at_random_ep_len=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[name].append(dict(ms_per_iteration=dt / iters * 1e3, env_steps_per_s=r.num_steps_per_env * num_envs * iters / dt,
                                  rollout_ms=r.last_collection_time * 1e3, update_ms=r.last_learn_time * 1e3))
    out["graphs"] = {name: (r._graph is not None, r._update_graph is not None) for name, r in runners.items()}
    return out, runners


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


def parts_cost(runner):
    import hgym
    alg = runner.alg
    g, st, net = alg._guide, alg.storage, alg.net
    T, N = st.num_transitions_per_env, st.num_envs
    mb = T * N // alg.num_mini_batches
    with torch.inference_mode():
        idx = torch.randperm(T * N, device="cuda")[:mb].contiguous()
        sh = st.shadows(mirrored=False)
        kw = dict(obs_bf16=sh[0], priv_bf16=sh[1]) if sh is not None else {}
        batch = hgym.make_batch(*st.batch_columns(), idx, **kw)
        guided = g.minibatch()
        out = dict(rows=T * N, minibatch=mb, teacher_max_batch=int(g.tnet.cfg.max_batch), shadow=sh is not None,
                   teacher_pass_us=_median_us(lambda: g.teacher_pass(st)),
                   schedule_us=_median_us(lambda: hgym.guide_schedule(g.struct, g.count_dev, g.coef)),
                   grad_plain_us=_median_us(lambda: net.ppo_grad(alg._ppo_cfg, batch)),
                   grad_guide_us=_median_us(lambda: net.ppo_grad_guide(alg._ppo_cfg, batch, guided)))
    return out


if __name__ == "__main__":
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    runs, runners = runs_cost(num_envs, iters, legs)
    print(json.dumps(dict(num_envs=num_envs, iters=iters, legs=legs, runs=runs, parts=parts_cost(runners["on"])), indent=1))
