"""Same-call A/B of an evaluation of N envs x T steps: OnPolicyRunner.evaluate on the fused, captured path against the same steps as a
Python loop over act_inference + env.step (the pieces that existed before the evaluation launch).  One evaluation is a few
milliseconds, so a sample is a block of 50 back-to-back evaluations between two HIP events; the two paths alternate, three samples each,
after a warm-up evaluation of each (the fused path: three, so that the graph is captured and has replayed once).

    python tools/eval_rollout_ab.py [--envs 4096] [--steps 60] [--block 50] > profiles/eval_rollout_ab.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "humanoid-gym_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--block", type=int, default=50)
    a = ap.parse_args()
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    mk = lambda n: get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(n), "--seed", "1"])
    args = mk(max(32, (-(-a.envs * 4 // 60) + 31) // 32 * 32))
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    ev_args = mk(a.envs)
    ev, _ = task_registry.make_env(name=ev_args.task, args=ev_args)
    ac = runner.alg.actor_critic
    assert ev.eval_rollout_supported(runner.alg.net), "the fused evaluation launch does not serve this env / policy"

    def fused():
        return runner.evaluate(ev, a.steps)

    def loop():
        with torch.inference_mode():
            obs, _ = ev.reset()
            for _ in range(a.steps):
                obs = ev.step(ac.act_inference(obs))[0]
            return float(ev.rew_buf.sum())          # one read-back, as evaluate() has

    def fallback():          # (for information: evaluate()'s own two-launch path, the loop + the accumulator launch behind every step)
        return runner.evaluate(ev, a.steps, fused=False)

    for _ in range(3):
        fused()
    loop()
    fallback()
    assert runner._eval_capture.graph is not None
    ms = {"fused": [], "loop": [], "fallback": []}
    for _ in range(3):
        for name, fn in (("fused", fused), ("loop", loop), ("fallback", fallback)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.block):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.block)
    print("command: python tools/eval_rollout_ab.py --envs %d --steps %d --block %d" % (a.envs, a.steps, a.block))
    print("device: %s; ms per evaluation (reset + %d vec-steps of %d envs + one read-back), blocks of %d, paths alternating" % (
        torch.cuda.get_device_name(0), a.steps, a.envs, a.block))
    for name in ("fused", "loop", "fallback"):
        v = ms[name]
        print("%-8s samples %s  median %.3f  spread (max - min) %.3f" % (name, " ".join("%.3f" % x for x in v), statistics.median(v), max(v) - min(v)))
    mf, ml = statistics.median(ms["fused"]), statistics.median(ms["loop"])
    print("fused / loop = %.3f; requirement (fused median <= loop median + loop spread): %s" % (
        mf / ml, "met" if mf <= ml + (max(ms["loop"]) - min(ms["loop"])) else "NOT met"))


if __name__ == "__main__":
    main()
