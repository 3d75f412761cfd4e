"""How good is a checkpoint: OnPolicyRunner.evaluate on the policy's mean actions over many robots, printed as one JSON line.

    python humanoid/scripts/evaluate.py --task=humanoid_ppo --load_run <run> --checkpoint <it> --num_envs 4096 --steps 600

play.py answers "does it walk" for one robot; this answers "mean episode return / fall rate / velocity-tracking error over --num_envs
robots".  Same overrides of the test configuration as play.py (:50-66) except the env count.  Every vec-step is one fused launch where
the env and the policy allow it (LeggedRobot.eval_rollout_supported), the whole evaluation one replayed HIP graph."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from humanoid.envs import *  # noqa: F401,F403,E402
from humanoid.utils import get_args, task_registry  # noqa: E402


def eval_overrides(env_cfg, num_envs):
    """play.py's overrides of the test configuration (:50-66), with the env count of the evaluation."""
    env_cfg.env.num_envs = int(num_envs)
    env_cfg.terrain.mesh_type = "plane"
    env_cfg.terrain.num_rows = 5
    env_cfg.terrain.num_cols = 5
    env_cfg.terrain.curriculum = False
    env_cfg.terrain.max_init_terrain_level = 5
    env_cfg.noise.add_noise = True
    env_cfg.domain_rand.push_robots = False
    env_cfg.domain_rand.joint_angle_noise = 0.0
    env_cfg.noise.curriculum = False
    env_cfg.noise.noise_level = 0.5
    return env_cfg


def evaluate(args, steps=600, num_envs=None):
    import copy
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    env_cfg, train_cfg = copy.deepcopy(env_cfg), copy.deepcopy(train_cfg)
    num_envs = int(num_envs if num_envs is not None else (args.num_envs or env_cfg.env.num_envs))
    args.num_envs = None                                   # (update_cfg_from_args would put it into both envs)
    eval_cfg = eval_overrides(copy.deepcopy(env_cfg), num_envs)
    train_cfg.seed = 123145
    # the runner wants an env of its own; the policy's batch limit (HgymNetConfig.max_batch) is never below that env's count, so an env
    # of the evaluation's size makes a net that takes the evaluation's rows in one call
    env_cfg = eval_overrides(env_cfg, num_envs)
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = True
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg, log_root=None)
    eval_env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=eval_cfg)
    runner.alg.actor_critic.eval()
    if not eval_env.eval_rollout_supported(runner.alg.net):
        print("evaluate.py: this env / policy takes the two-launch path (LeggedRobot.eval_rollout_supported is False)", file=sys.stderr)
    return runner.evaluate(eval_env, steps)


if __name__ == "__main__":
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--steps", type=int, default=600)
    own, rest = p.parse_known_args()
    result = evaluate(get_args(rest), steps=own.steps)
    print(json.dumps(result))
