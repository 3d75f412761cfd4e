"""What critic-only training costs at the training script's size (profiles/critic_only_cost.txt).  Cost only.

One process: two distillation runners (humanoid_distill, Distillation.train_critic off / on) and a PPO runner (humanoid_ppo), all at
num_envs x 60 steps with minibatches of 15 steps' rows.

  loops    learn(iters) of the two distillation runners, legs alternating: ms per iteration by a host clock around a device synchronise,
           and the runner's own split into rollout and update.
  calls    HIP events around eager calls on the rows the last rollout left, the median of `reps`: hgym_bc_vf_grad against hgym_bc_grad
           alone and against hgym_bc_grad + hgym_vf_grad(keep_others = 1) in sequence; one hgym_vf_grad against one hgym_ppo_grad at the
           same B on the PPO runner's rows.

python tools/critic_only_cost.py [num_envs] [iters] [legs] [reps]"""
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

RUNS = ("off", "on")


def _runner(task, num_envs, train_critic=False):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + task, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=task))
    if train_critic:
        train_cfg.algorithm.train_critic = True
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


def calls_cost(distill, ppo, reps):
    import hgym
    out = {}
    alg, st, net = distill.alg, distill.alg.storage, distill.alg.net
    T, N = st.num_transitions_per_env, st.num_envs
    mb = alg.gradient_length * N
    with torch.inference_mode():
        st.shadow_valid = [True] * T            # the last rollout's shadows are still there; update() only cleared the flags
        sh = st.shadows()
        cols = st.batch_columns()
        obs, target, rows = cols[0], st.teacher_actions.flatten(0, 1), alg._rows[:mb]
        z = lambda: torch.zeros(2, dtype=torch.float64, device=obs.device)
        bc_sums, vf_sums = z(), z()
        kw = {} if sh is None else dict(priv_bf16=sh[1])
        bc_batch = hgym.make_bc_batch(obs, rows, None if sh is None else sh[0])
        vf_batch = hgym.make_vf_batch(cols[1], cols[3], cols[5], rows, **kw)
        both = hgym.make_vf_batch(cols[1], cols[3], cols[5], rows, obs=obs, obs_bf16=None if sh is None else sh[0], **kw)
        vf_keep = hgym.make_vf_config(alg.clip_param, alg.value_loss_coef, keep_others=True)

        def in_sequence():
            net.bc_grad(alg._bc_cfg, bc_batch, target, bc_sums)
            net.vf_grad(vf_keep, vf_batch, vf_sums)
        out["bc_grad"] = _median_us(lambda: net.bc_grad(alg._bc_cfg, bc_batch, target, bc_sums), reps)
        out["bc_grad_then_vf_grad"] = _median_us(in_sequence, reps)
        out["bc_vf_grad"] = _median_us(lambda: net.bc_vf_grad(alg._bc_cfg, alg._vf_cfg, both, target, bc_sums, vf_sums), reps)
        out["rows"], out["shadow"] = mb, sh is not None
        # one hgym_vf_grad against one hgym_ppo_grad on the PPO runner's rows, the same B
        palg, pst = ppo.alg, ppo.alg.storage
        pst.shadow_valid = [True] * T
        psh = pst.shadows()
        pcols = pst.batch_columns()
        idx = torch.arange(mb, dtype=torch.int64, device=obs.device)
        assert int(palg.net.cfg.max_batch) == mb, (int(palg.net.cfg.max_batch), mb)
        pbatch = hgym.make_batch(*pcols, idx, **({} if psh is None else dict(obs_bf16=psh[0], priv_bf16=psh[1])))
        pvf = hgym.make_vf_batch(pcols[1], pcols[3], pcols[5], idx, **({} if psh is None else dict(priv_bf16=psh[1])))
        vf_alone = hgym.make_vf_config(palg.clip_param, palg.value_loss_coef)
        out["ppo_grad"] = _median_us(lambda: palg.net.ppo_grad(palg._ppo_cfg, pbatch), reps)
        out["vf_grad"] = _median_us(lambda: palg.net.vf_grad(vf_alone, pvf, vf_sums), reps)
        out["ppo_apply"] = _median_us(lambda: palg.net.ppo_apply(palg._ppo_cfg), reps)
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "critic_only_cost.py measures on the GPU; none visible"
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 4096
    iters = int(argv[1]) if len(argv) > 1 else 20
    legs = int(argv[2]) if len(argv) > 2 else 3
    reps = int(argv[3]) if len(argv) > 3 else 30
    ppo = _runner("humanoid_ppo", n)
    runners = dict(off=_runner("humanoid_distill", n), on=_runner("humanoid_distill", n, train_critic=True))
    teacher = {k: v.detach().clone() for k, v in ppo.alg.actor_critic.state_dict().items()}
    for r in runners.values():
        assert r.alg.actor_critic.load_state_dict(teacher) is False      # the PPO runner's actor as the teacher
    for r in list(runners.values()) + [ppo]:
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)        # eager, capture, replays
    torch.cuda.synchronize()
    res = dict(num_envs=n, iters=iters, legs=legs, loops=loops_cost(runners, n, iters, legs))
    res["calls"] = calls_cost(runners["on"], ppo, reps)
    print(json.dumps(res, indent=1), flush=True)
