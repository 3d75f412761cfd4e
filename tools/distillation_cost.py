"""What distillation (Distillation / StudentTeacher, hgym_bc_grad) costs at the training script's size (profiles/distillation_cost.txt).

One process, a PPO runner (humanoid_ppo) and a distillation runner (humanoid_distill) side by side, both at num_envs x 60 steps with
minibatches of 15 steps' rows (PPO: 4 minibatches; Distillation: gradient_length 15):

  calls    HIP events around eager calls on the rows the last rollout left, medians over `reps`: hgym_bc_grad (the student's tiles with the
           regression head, the scalars, the actor's four weight-gradient products, the actor's slab sums), hgym_ppo_grad at the same B (both
           nets), hgym_ppo_apply behind each, and the teacher's pass over the T N rows (Distillation.compute_returns).
  loops    learn(iters) of either runner, legs alternating: ms per iteration by a host clock around a device synchronise, and the runner's own
           split into rollout and update.

python tools/distillation_cost.py [num_envs] [iters] [legs] [reps]"""
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


def _runner(task, num_envs):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + task, "--headless", "--num_envs", str(num_envs), "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=task))
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    return runner


def _teacher_into(distill, ppo):
    """The PPO runner's actor as the teacher (its widths are the task's teacher_hidden_dims)."""
    sd = {k: v.detach().clone() for k, v in ppo.alg.actor_critic.state_dict().items()}
    assert distill.alg.actor_critic.load_state_dict(sd) is False


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


def _mlp_flops(dims, rows):
    """Algorithmic flops of a cloning / PPO minibatch over one MLP: forward 2, dX 2 (not for the first layer), dW 2 per weight and row."""
    fwd = sum(2.0 * rows * a * b for a, b in zip(dims, dims[1:]))
    return fwd + (fwd - 2.0 * rows * dims[0] * dims[1]) + fwd


def calls_cost(ppo, distill, reps):
    import hgym
    out = {}
    # --- hgym_bc_grad on the distillation runner's rows
    alg, st = distill.alg, distill.alg.storage
    T, N = st.num_transitions_per_env, st.num_envs
    mb = alg.gradient_length * N
    st.shadow_valid = [True] * T            # the last rollout's shadows are still there; update() only cleared the flags
    sh = st.shadows()
    obs, target = st._obs_all[:T].flatten(0, 1), st.teacher_actions.flatten(0, 1)
    sums = torch.zeros(2, dtype=torch.float64, device=obs.device)
    batch = hgym.make_bc_batch(obs, alg._rows[:mb], None if sh is None else sh[0])
    out["bc_grad"] = _median_ms(lambda: alg.net.bc_grad(alg._bc_cfg, batch, target, sums), reps)
    out["bc_apply"] = _median_ms(lambda: alg.net.ppo_apply(alg._ppo_cfg), reps)
    out["teacher_pass"] = _median_ms(lambda: alg.compute_returns(None), reps)
    ac = alg.actor_critic
    sdims = [ac.num_actor_obs] + ac.student_hidden_dims + [ac.num_actions]
    tdims = [ac.num_actor_obs] + ac.teacher_hidden_dims + [ac.num_actions]
    out["bc_grad"]["rows"], out["bc_grad"]["flops"] = mb, _mlp_flops(sdims, mb)
    # gathered bf16 rows in, the three hidden activations and four dZ out and in again for the weight gradients, the slabs
    ld = alg.net.shadow_ld(0)
    out["bc_grad"]["bytes"] = mb * (2.0 * ld + 12 * 4 + 2 * 2.0 * (sum(sdims[1:-1]) + sum(sdims[1:-1]) + 32)) + 9.0 * 4 * (alg.net.bucket_split - 12)
    out["teacher_pass"]["rows"] = T * N
    out["teacher_pass"]["flops"] = sum(2.0 * T * N * a * b for a, b in zip(tdims, tdims[1:]))
    out["teacher_pass"]["bytes"] = T * N * (4.0 * tdims[0] + 4.0 * tdims[-1])
    # --- hgym_ppo_grad at the same B on the PPO runner's rows
    palg, pst = ppo.alg, ppo.alg.storage
    pst.shadow_valid = [True] * T
    psh = pst.shadows()
    idx = torch.arange(mb, dtype=torch.int64, device=obs.device)
    pbatch = hgym.make_batch(*pst.batch_columns(), idx, **({} if psh is None else dict(obs_bf16=psh[0], priv_bf16=psh[1])))
    assert int(palg.net.cfg.max_batch) == mb, (int(palg.net.cfg.max_batch), mb)
    out["ppo_grad"] = _median_ms(lambda: palg.net.ppo_grad(palg._ppo_cfg, pbatch), reps)
    out["ppo_apply"] = _median_ms(lambda: palg.net.ppo_apply(palg._ppo_cfg), reps)
    pa = palg.actor_critic
    out["ppo_grad"]["rows"] = mb
    out["ppo_grad"]["flops"] = (_mlp_flops([pa.num_actor_obs] + pa.actor_hidden_dims + [pa.num_actions], mb) +
                                _mlp_flops([pa.num_critic_obs] + pa.critic_hidden_dims + [1], mb))
    out["shadows"] = dict(bc=sh is not None, ppo=psh is not None)
    for k in ("bc_grad", "teacher_pass", "ppo_grad"):
        out[k]["tflops"] = out[k]["flops"] / (out[k]["median_ms"] * 1e-3) / 1e12
        if "bytes" in out[k]:
            out[k]["gbytes_per_s"] = out[k]["bytes"] / (out[k]["median_ms"] * 1e-3) / 1e9
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
    assert torch.cuda.is_available(), "distillation_cost.py measures on the GPU; none visible"
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 4096
    iters = int(argv[1]) if len(argv) > 1 else 20
    legs = int(argv[2]) if len(argv) > 2 else 3
    reps = int(argv[3]) if len(argv) > 3 else 21
    runners = dict(ppo=_runner("humanoid_ppo", n), distill=_runner("humanoid_distill", n))
    _teacher_into(runners["distill"], runners["ppo"])
    for r in runners.values():
        r.learn(num_learning_iterations=4, init_at_random_ep_len=True)        # eager, capture, replays
    torch.cuda.synchronize()
    res = dict(num_envs=n, loops=loops_cost(runners, n, iters, legs))
    res["calls"] = calls_cost(runners["ppo"], runners["distill"], reps)
    print(json.dumps(res, indent=1), flush=True)
